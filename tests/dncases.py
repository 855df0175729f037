"""The denoiser's test cases, shared by tests/test_denoise_ref.py (the restatement's own properties and the tie cap of every case,
CPU) and tests/test_denoise.py (the device against the restatement).  All at 24 kHz.

Signals: the six of tests/test_spectrogram.py plus noise_330 (uniform +-330) and tone_noise (8000 sin at 1 kHz plus uniform +-100).
A case is (frame N, clip length n, signal names, preset); its seed is changed, never the cap, if its signals trip the tie cap."""
import functools

import numpy as np

import dnref
from test_spectrogram import RATE, signal as spec_signal

EXTRA = ("noise_330", "tone_noise")


@functools.lru_cache(maxsize=None)
def signal(name, n, seed=0):
    """int16 [n] at 24 kHz, seeded, read-only."""
    if name not in EXTRA:
        return spec_signal(name, n, seed)
    rng = np.random.default_rng([seed, 100 + EXTRA.index(name), n])
    if name == "noise_330":
        x = rng.integers(-330, 331, n)
    else:
        x = np.round(8000.0 * np.sin(2.0 * np.pi * 1000.0 * np.arange(n) / RATE)) + rng.integers(-100, 101, n)
    x = x.astype(np.int16)
    x.setflags(write=False)
    return x


ABOVE_FLOOR = ("noise_330", "chirp", "tone_noise", "noise_full", "impulse", "silence")      # usable at every preset
PRESET_N, PRESET_LEN = 1024, 5 * 1024 + 77                                                 # frame_for_rate(24000); 21 hops, a partial one

# name -> (N, n, signals, preset, seed)
CASES = {}
for _N in (64, 128, 256, 512, 1024, 2048, 4096):                                           # every pass structure
    CASES[f"passes_{_N}"] = (_N, 10 * _N + 3, ("noise_full",), "medium", 0)
CASES["tiles_many"] = (64, 5000, ("noise_full", "chirp", "tone_noise"), "medium", 0)       # 313 hops: many tiles, a partial tile and hop, 3 clips
CASES["tiles_exact"] = (256, 16 * 64, ("noise_full",), "medium", 0)                        # n = 16 h
CASES["below_hop"] = (64, 7, ("noise_full",), "medium", 0)
CASES["one_sample"] = (64, 1, ("noise_full",), "medium", 0)
for _p in dnref.PRESETS:
    CASES[f"preset_{_p}"] = (PRESET_N, PRESET_LEN, ABOVE_FLOOR + (("noise_33",) if _p != "heavy" else ()), _p, 0)


@functools.lru_cache(maxsize=None)
def clips(case):
    """int16 [B, n] of a case, read-only."""
    N, n, names, preset, seed = CASES[case]
    x = np.stack([signal(s, n, seed) for s in names])
    x.setflags(write=False)
    return x


def params(case):
    """(N, nr_db, nf_db)"""
    N, _, _, preset, _ = CASES[case]
    return (N,) + tuple(float(v) for v in dnref.PRESETS[preset])


@functools.lru_cache(maxsize=None)
def restated(case):
    """(int16 [B, n], v float64 [B, n]) of a case: computed once, shared, read-only."""
    q, v = dnref.denoise_pcm16(clips(case), *params(case))
    q.setflags(write=False)
    v.setflags(write=False)
    return q, v
