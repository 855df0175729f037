"""The inputs of the FLAC LPC tests, shared by the CPU tests of the restatement (test_flac_lpc_ref.py) and the device tests
(test_flac_lpc.py): 4096-sample contents that each reach one branch of the LPC analysis, and the batches built from them.  Every
case is built once, encoded once by the restatement (tests/flaclpcref.py), and never changed."""
import functools

import numpy as np

import flaclpcref
import loudref

B = flaclpcref.BLOCK
LENGTHS = (1, 2, 3, 5, 9, 16, 17, 64, 255, 256, 257, 4095, 4096, 4097, 8225)


def _rng(seed):
    return np.random.default_rng(seed)


def _i16(v):
    return np.clip(np.round(v), -32768, 32767).astype(np.int16)


def _ar(order, scale=50.0, gains=None):
    """An all-pole source of `order` poles (pairs at radius 0.9..0.98, a real one for an odd order) driven by white noise."""
    rng = _rng(100 * order)
    poles = []
    for _ in range(order // 2):
        r, th = 0.9 + 0.08 * rng.random(), 0.2 + 2.6 * rng.random()
        poles += [r * np.exp(1j * th), r * np.exp(-1j * th)]
    if order % 2:
        poles.append(-0.9)
    a = np.poly(poles).real[1:]
    e = _rng(0).standard_normal(B + 200) * scale
    y = np.zeros(B + 200)
    for i in range(order, B + 200):
        y[i] = e[i] - sum(a[j] * y[i - 1 - j] for j in range(order))
    y = y[200:]
    return _i16(y if gains is None else y * np.repeat(np.resize(np.array(gains, np.float64), 8), B // 8))


def _at(i, v):
    x = np.zeros(B, np.int16)
    x[i] = v
    return x


# name: (builder, the branch it is there for: the frame's kind and, where LPC, its order (or None))
CONTENTS = {f"ar{p}": (functools.partial(_ar, p), ("LPC", p)) for p in range(1, 9)}
CONTENTS.update({
    "ar2_steps": (lambda: _ar(2, 4.0, [1, 30, 300, 3]), ("LPC", None)),            # partition orders above 0
    "noise3": (lambda: _i16(_rng(3).integers(-3, 4, B)), ("FIXED",)),               # near-white, low level: shift 15 after the clamp
    "full_scale": (lambda: _i16(_rng(2).integers(-32768, 32768, B)), ("VERBATIM",)),
    "zeros": (lambda: np.zeros(B, np.int16), ("CONSTANT",)),
    "one_at_0": (lambda: _at(0, 1), ("FIXED",)),                                     # the window takes it to zero: R[0] == 0
    "spike": (lambda: _at(2000, 1000), ("FIXED",)),                                  # R[l] == 0 above l = 0: every coefficient zero
})


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
    s = 300 + (37 * i) % B
    return x[s:s + n]


def _cases():
    c = {}
    # name: (rate, clips [Bc, n], factor or None, seek_interval, lpc_order)
    c["contents_one_clip"] = (48000, np.concatenate([content(k) for k in CONTENTS] + [content("ar3")[:33]])[None, :], None, 3000, 8)
    for j, n in enumerate(LENGTHS):
        c[f"len{n}"] = (48000, np.stack([_mix(n, i) for i in range(3)]), None if n % 2 else np.array([1.0, 0.5, 2.75]), 48000 if n > 4096 else 0,
                        (8, 4, 1)[j % 3])
    c["contents_order4"] = (32000, c["contents_one_clip"][1], None, 0, 4)
    c["contents_order1"] = (8000, c["contents_one_clip"][1][:, :6 * B + 17], np.array([0.7]), 8000, 1)
    c["sixty_five"] = (32000, np.stack([_mix(4097, i) for i in range(65)]), np.where(np.arange(65) % 3 == 1, 0.37, 1.0), 4096, 8)
    return c


CASES = _cases()
for _v in CASES.values():
    _v[1].setflags(write=False)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (all streams back to back, offsets uint64 [Bc + 1], per clip the restatement's per-frame info, the gained clips)"""
    rate, clips, factor, seek, lpc_order = CASES[name]
    gained = [c if factor is None else loudref.apply_gain(c, float(factor[i])) for i, c in enumerate(clips)]
    enc = [flaclpcref.encode(g, rate, seek, lpc_order, info=True) for g in gained]
    offsets = np.concatenate([[0], np.cumsum([len(s) for s, _ in enc])]).astype(np.uint64)
    return b"".join(s for s, _ in enc), offsets, [i for _, i in enc], gained


def owl_pcm16(golden_dir):
    """The first 40 frames of the reference's tawny-owl recording at 16 bits."""
    import os
    z = np.load(os.path.join(golden_dir, "tawnyowl_pcm32.npz"))
    acc = np.cumsum(z["delta"].astype(np.int64))
    return (((acc + 2**31) % 2**32 - 2**31) >> 16).astype(np.int16)[:40 * 4096]
