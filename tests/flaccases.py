"""The inputs of the FLAC tests, shared by the CPU tests of the restatement (test_flac_ref.py) and the device tests (test_flac.py):
fourteen 4096-sample contents that each reach one branch of the encoder, and the batches built from them.  Every case is built once,
encoded once by the restatement, and never changed."""
import functools

import numpy as np

import flacref

B = flacref.BLOCK


def _rng(seed):
    return np.random.default_rng(seed)


def _i16(v):
    return np.clip(np.round(v), -32768, 32767).astype(np.int16)


def _steps(parts):
    """+-1 noise scaled by [1, 30, 900, 9000] in turn over `parts` equal runs of the block."""
    scale = np.repeat(np.resize(np.array([1, 30, 900, 9000]), parts), B // parts)
    return _i16(_rng(20 + parts).integers(-1, 2, B) * scale)


def _gated():
    x = _rng(31).integers(-3000, 3001, B)
    x[(np.arange(B) // 128) % 7 != 0] = 0
    return _i16(x)


def _single_one():
    x = np.zeros(B, np.int16)
    x[1000] = 1
    return x


t = np.arange(B)
# name: (builder, the branch it is there for: kind, and where FIXED (order, porder or None, a k that must appear or None))
CONTENTS = {
    "noise20000": (lambda: _i16(_rng(1).integers(-20000, 20001, B)), ("FIXED", 0, None, 14)),
    "full_scale": (lambda: _i16(_rng(2).integers(-32768, 32768, B)), ("VERBATIM",)),
    "noise3": (lambda: _i16(_rng(3).integers(-3, 4, B)), ("FIXED", 0, None, 1)),
    "walk40": (lambda: _i16(np.cumsum(_rng(4).integers(-40, 41, B))), ("FIXED", 1, None, None)),
    "double_walk2": (lambda: _i16(np.cumsum(np.cumsum(_rng(2).integers(-2, 3, B)))), ("FIXED", 2, 3, None)),
    "sine100": (lambda: _i16(30000.0 * np.sin(2.0 * np.pi * 100.0 * t / 48000.0)), ("FIXED", 3, None, 0)),
    "sine1k_noise2": (lambda: _i16(np.round(20000.0 * np.sin(2.0 * np.pi * 1000.0 * t / 48000.0)) + _rng(7).integers(-2, 3, B)), ("FIXED", 4, None, None)),
    "steps2": (lambda: _steps(2), ("FIXED", None, 1, None)),
    "steps4": (lambda: _steps(4), ("FIXED", None, 2, None)),
    "steps8": (lambda: _steps(8), ("FIXED", None, 3, None)),
    "steps16": (lambda: _steps(16), ("FIXED", None, 4, None)),
    "gated7": (_gated, ("FIXED", None, 5, None)),
    "zeros": (lambda: np.zeros(B, np.int16), ("CONSTANT",)),
    "single_one": (_single_one, ("FIXED", 0, None, 0)),
}
LENGTHS = (1, 2, 3, 5, 16, 17, 255, 256, 257, 4095, 4096, 4097, 8192 + 33)
RATES = (48000, 32000, 24000, 256000, 11025)


@functools.lru_cache(maxsize=None)
def content(name):
    x = CONTENTS[name][0]()
    assert x.dtype == np.int16 and x.shape == (B,)
    x.setflags(write=False)
    return x


def _mix(n, i):
    """Clip i of a batch of length n: the contents in turn, starting at another one and another sample each time."""
    names = list(CONTENTS)
    need = n // B + 2
    x = np.concatenate([content(names[(i + j * 5) % len(names)]) for j in range(need)])
    s = (37 * i) % B
    return x[s:s + n]


def _long(frames, extra, active):
    x = np.zeros(frames * B + extra, np.int16)
    x[active * B:(active + 1) * B] = content("walk40")
    x[-1] = -7 if extra else x[-1]
    return x


def _cases():
    c = {}
    # name: (rate, clips [Bc, n], factor or None, seek_interval)
    c["contents_one_clip"] = (48000, np.concatenate([content(k) for k in CONTENTS] + [content("sine100")[:33]])[None, :], None, 3000)
    for n in LENGTHS:
        c[f"len{n}"] = (48000, np.stack([_mix(n, i) for i in range(3)]), None if n % 2 else np.array([1.0, 0.5, 2.75]), 48000 if n > 4096 else 0)
    for r in RATES:
        c[f"rate{r}"] = (r, np.stack([_mix(4096 + 300, i + 3) for i in range(3)]), None, r // 8)
    c["sixty_five"] = (32000, np.stack([_mix(B + 257, i) for i in range(65)]), np.where(np.arange(65) % 3 == 1, 0.37, 1.0), 4096)
    c["two_byte_numbers"] = (48000, _long(129, 7, 128)[None, :], None, 48000)
    c["three_byte_numbers"] = (24000, _long(2049, 1, 2047)[None, :], None, 0)
    return c


CASES = _cases()
for _v in CASES.values():
    _v[1].setflags(write=False)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (all streams back to back, offsets uint64 [Bc + 1], per clip the restatement's per-frame info, the gained clips)"""
    import loudref
    rate, clips, factor, seek = CASES[name]
    gained = [c if factor is None else loudref.apply_gain(c, float(factor[i])) for i, c in enumerate(clips)]
    enc = [flacref.encode(g, rate, seek, info=True) for g in gained]
    offsets = np.concatenate([[0], np.cumsum([len(s) for s, _ in enc])]).astype(np.uint64)
    return b"".join(s for s, _ in enc), offsets, [i for _, i in enc], gained
