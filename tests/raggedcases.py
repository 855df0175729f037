"""The bursts of the ragged-entry tests (test_ragged_ref.py on the CPU, test_flac_ragged.py and test_loudness_ragged.py on the
device): lists of int16 clips of unequal lengths at 8 kHz (S = 800, q = 8 for every call, the lanes nowhere near the cap).  Every
burst is built once, restated once per clip (flacref / flaclpcref / loudref), and never changed."""
import functools

import numpy as np

import flaclpccases
import flaclpcref
import flacref
import loudref

RATE = 8000
S = 800
SEEKS = (0, 8000)
LPC_ORDERS = (0, 4, 8)
EXPORT = dict(T=-23.0, C=-1.0, max_gain=60.0, gate_fallback=True)        # actions_database.go:1392-1438
UPLOAD = dict(T=-23.0, C=-1.0, max_gain=30.0, gate_fallback=False)       # encode_native.go:25-66

# (a) n < S, one sub-block exactly, a trailing remainder; 1, 2, 3 and 4 frames, a short last frame and none; 1, 5, 9 and 13
# true-peak tiles; the shortest clips first and in the middle; odd lengths put later clips on odd sample offsets
LENS_A = (1, 799, 800, 801, 4095, 4096, 4097, 8225, 37, 12289)
# (b) crosses the 64-clip block of the scan and the 256-thread block of the batch layout; most clips have no sub-block
LENS_B = tuple(1 + (7 * c) % 257 for c in range(300))
# (c) one length: the shape of the uniform fused test
LENS_C = (5 * S + 37,) * 5
# (d) test_flac.loud_batch cut short: the gate lift's second run happens on a strict subset of the burst
LENS_D = (4037, 3200, 4037, 2400 + 1, 4037)


def _i16(v):
    return np.clip(np.round(v), -32768, 32767).astype(np.int16)


def _tone(n, hz, amp, phase=0.0):
    return _i16(amp * 32767.0 * np.sin(2.0 * np.pi * hz * np.arange(n) / RATE + phase))


def _noise(seed, n, amp):
    return _i16(np.random.default_rng(seed).standard_normal(n) * amp * 32768.0)


def loud_batch(n, count):
    """test_flac.loud_batch at 8 kHz: tones and noises of several levels, a sub-gate clip and silence."""
    rng = np.random.default_rng(77)
    t = np.arange(n)
    rows = []
    for i in range(count):
        amp = (0.6, 0.02, 0.0004, 0.2, 0.0)[i % 5]
        x = amp * 32767.0 * (np.sin(2.0 * np.pi * (200.0 + 90.0 * i) * t / RATE) if i % 2 == 0 else rng.standard_normal(n) / 3.0)
        rows.append(np.clip(np.round(x), -32768, 32767).astype(np.int16))
    return np.stack(rows)


def _burst_a():
    n = LENS_A
    return [np.array([17], np.int16), _noise(1, n[1], 0.05), _tone(n[2], 440.0, 0.3), np.full(n[3], 1234, np.int16), _noise(4, n[4], 0.1),
            np.zeros(n[5], np.int16), _tone(n[6], 310.0, 0.5, 0.7), np.ascontiguousarray(flaclpccases._mix(n[7], 3)), _noise(8, n[8], 0.3),
            np.ascontiguousarray(flaclpccases._mix(n[9], 1))]


def _burst_b():
    out = []
    for c, n in enumerate(LENS_B):
        kind = c % 4
        out.append(_noise(100 + c, n, 0.2) if kind == 0 else _tone(n, 150.0 + 11.0 * c, 0.4, 0.1 * c) if kind == 1 else
                   np.full(n, -7 * c, np.int16) if kind == 2 else np.zeros(n, np.int16))
    return out


def _burst_c():
    return list(loud_batch(LENS_C[0], 5))


def _burst_d():
    return [x[:n].copy() for x, n in zip(loud_batch(4037, 5), LENS_D)]


BUILDERS = {"a": (LENS_A, _burst_a), "b": (LENS_B, _burst_b), "c": (LENS_C, _burst_c), "d": (LENS_D, _burst_d)}


@functools.lru_cache(maxsize=None)
def burst(name):
    lens, build = BUILDERS[name]
    clips = build()
    assert tuple(c.size for c in clips) == tuple(lens) and all(c.dtype == np.int16 and c.ndim == 1 for c in clips)
    for c in clips:
        c.setflags(write=False)
    return tuple(clips)


def factors(name):
    """One gain per clip: the identity, a cut and a boost that saturates loud clips, in turn."""
    return np.array([(1.0, 0.37, 2.75)[c % 3] for c in range(len(BUILDERS[name][0]))], np.float64)


def encode_one(x, seek, lpc_order):
    x = np.ascontiguousarray(x)
    return flaclpcref.encode(x, RATE, seek, lpc_order) if lpc_order else flacref.encode(x, RATE, seek)


@functools.lru_cache(maxsize=None)
def flac_reference(name, lpc_order, seek, with_factor):
    """-> (the restated stream of every clip, the gained clips)"""
    fac = factors(name) if with_factor else None
    gained = [c if fac is None else loudref.apply_gain(c, float(fac[i])) for i, c in enumerate(burst(name))]
    return tuple(encode_one(g, seek, lpc_order) for g in gained), tuple(gained)


@functools.lru_cache(maxsize=None)
def measurements(name):
    """The restatement's measurement of every clip."""
    return tuple(loudref.measure(c, RATE) for c in burst(name))
