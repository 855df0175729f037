"""The streams of the recording decoder's tests (tests/flacwidemux.py writes them): cases() -> name -> (stream, samples [frames,
channels], bits), every one valid; damaged() -> name -> (stream, status, frames, fail_offset, samples with zeros where nothing is
restored, bits).  Built once per process."""
import functools

import numpy as np

import flacwidemux as M

RATE = 48000
ASSIGN = {1: "independent", 8: "left_side", 9: "side_right", 10: "mid_side"}


def signal(n, channels, bits, seed, scale=0.25):
    """Correlated channels: a tone and noise, channel 1 a quieter copy with noise of its own."""
    rng = np.random.default_rng(seed)
    full = 1 << (bits - 1)
    t = np.arange(n)
    a = scale * full * np.sin(2 * np.pi * (300.0 + 40.0 * seed) * t / RATE) + rng.normal(0.0, full / 2000.0, n)
    cols = [a, 0.8 * a + rng.normal(0.0, full / 1500.0, n)][:channels]
    return np.clip(np.round(np.stack(cols, axis=1)), -full, full - 1).astype(np.int64)


def lpc(order, precision=12, shift=10):
    """A predictor of that order: 0.95 times the mean of the last `order` samples."""
    c = int(round(0.95 * (1 << shift) / order))
    return dict(kind="LPC", order=order, precision=precision, shift=shift, coefs=[c] * order)


def sub_kinds():
    """Every subframe kind the issue names, as (name, spec)."""
    out = [("constant", dict(kind="CONSTANT")), ("verbatim", dict(kind="VERBATIM"))]
    out += [(f"fixed{o}", dict(kind="FIXED", order=o)) for o in range(5)]
    out += [(f"lpc{o}", lpc(o)) for o in (1, 8, 9, 32)]
    out += [("rice_method1", dict(kind="FIXED", order=2, method=1, porder=2)), ("escape", dict(kind="FIXED", order=1, porder=1, ks=[("esc", 6), None])),
            ("rice_method0", dict(kind="FIXED", order=2, method=0)),
            ("partitions", dict(kind="FIXED", order=3, porder=3))]
    return out


def _kinds_stream(bits, assign):
    """One frame per kind in channel 0 with the next kind in channel 1 (so both channels take every kind), 64 samples a frame."""
    kinds, bs = sub_kinds(), 64
    x = signal(bs * len(kinds), 2, bits, 3 + bits, scale=0.02)      # (quiet: the crude predictors stay below the VERBATIM bound)
    frames = []
    for j, (name, spec) in enumerate(kinds):
        other = kinds[(j + 1) % len(kinds)][1]
        for s, col in ((spec, 0), (other, 1)):
            if s["kind"] == "CONSTANT":
                x[j * bs:(j + 1) * bs, col] = 1234 + col
            if s.get("ks"):                                          # the escape partition's residuals fit its 6 bits
                x[j * bs:j * bs + bs // 2, col] = -77 - col + 3 * (np.arange(bs // 2) % 5)
        frames.append(dict(assign=assign, subs=[spec, other]))
    if assign != 1:                                  # (the coded channels are not the samples: no constants or narrow escapes there)
        frames = [dict(assign=assign, subs=[_plain(f["subs"][0]), _plain(f["subs"][1])]) for f in frames]
    return M.stream(x, bits, bs, RATE, frames), x


def _plain(spec):
    return dict(kind="VERBATIM") if spec["kind"] == "CONSTANT" else dict(kind="FIXED", order=1) if spec.get("ks") else spec


def _extremes(bits, assign):
    full = 1 << (bits - 1)
    x = np.zeros((48, 2), np.int64)
    x[:16] = (full - 1, -full)                                       # side = 2^bits - 1: its 17th / 25th bit
    x[16:32] = (-full, full - 1)
    x[32:] = (full - 1, full - 1)
    return M.stream(x, bits, 16, RATE, dict(assign=assign, sub=dict(kind="VERBATIM"))), x


def _overflow24():
    """24-bit LPC of order 32 at precision 15 over near-full-scale alternating samples: one product is 2^37, the sum 2^42."""
    rng = np.random.default_rng(41)
    n = 192 * 2 + 40
    sign = np.where(np.arange(n) % 2 == 0, 1, -1)
    x = np.stack([sign * 8000000 + rng.integers(-100, 101, n), -sign * 7900000 + rng.integers(-100, 101, n)], axis=1).astype(np.int64)
    # (a coefficient with the sign of its sample adds 16383 x: the first two do, and of the other thirty half add and half take away)
    spec = dict(kind="LPC", order=32, precision=15, shift=15, method=1,
                coefs=[(16383 if j % 2 else -16383) * (1 if j < 17 else -1) for j in range(32)])
    return M.stream(x, 24, 192, RATE, dict(assign=1, sub=spec)), x


def _overflow24_window():
    """The same at order 8, the longest predictor the reader keeps in registers and the order of this project's encoder: precision
    15, near-full-scale alternating samples.  Five coefficients add 16383 x and three take it away, so one product is 2^37 and the
    sum of the five 2^39, the prediction (2 x 16383 / 2^15) x."""
    rng = np.random.default_rng(43)
    n = 192 * 2 + 40
    sign = np.where(np.arange(n) % 2 == 0, 1, -1)
    x = np.stack([sign * 8000000 + rng.integers(-100, 101, n), -sign * 7900000 + rng.integers(-100, 101, n)], axis=1).astype(np.int64)
    spec = dict(kind="LPC", order=8, precision=15, shift=15, method=1, porder=1,
                coefs=[(16383 if j % 2 else -16383) * (1 if j < 5 else -1) for j in range(8)])
    return M.stream(x, 24, 192, RATE, dict(assign=1, sub=spec)), x


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for bits in (16, 24):
        for assign, name in ASSIGN.items():
            x = signal(192 * 2 + 37, 2, bits, assign + bits)
            out[f"{name}_{bits}"] = (M.stream(x, bits, 192, RATE, dict(assign=assign)), x, bits)
            out[f"extremes_{name}_{bits}"] = _extremes(bits, assign) + (bits,)
            out[f"kinds_{name}_{bits}"] = _kinds_stream(bits, assign) + (bits,)
        x = np.stack([2 * np.arange(-40, 40) + 1, 2 * np.arange(80, 0, -1)], axis=1)        # every L + R is odd
        out[f"mid_side_odd_{bits}"] = (M.stream(x, bits, 16, RATE, dict(assign=10, sub=dict(kind="FIXED", order=1))), x, bits)
        x = signal(100, 2, bits, 5)
        x[:, 0] &= ~3
        x[:, 1] &= ~31
        out[f"wasted_{bits}"] = (M.stream(x, bits, 32, RATE, dict(assign=1, subs=[dict(kind="FIXED", order=2, wasted=2), dict(kind="VERBATIM", wasted=5)])),
                                 x, bits)
        x = signal(80, 2, bits, 6)
        x[:, 0] &= ~7
        x[:, 1] &= ~1
        out[f"wasted_side_{bits}"] = (M.stream(x, bits, 16, RATE, dict(assign=8, subs=[dict(kind="FIXED", order=1, wasted=3), dict(kind="FIXED", order=0, wasted=1)])),
                                      x, bits)
        x = signal(300, 1, bits, 7)
        out[f"mono_{bits}"] = (M.stream(x, bits, 64, RATE, dict(sub=lpc(8))), x, bits)
        for bs, total in ((16, 16 * 3 + 1), (16, 16 * 3 + 7), (192, 192 * 2 + 1), (192, 192 * 2 + 77), (4096, 4096 + 1), (4096, 4096 * 2 + 333)):
            x = signal(total, 2, bits, bs + total)
            assign = 10 if bs == 192 else 8
            spec = dict(assign=assign, sub=dict(kind="FIXED", order=2, porder=2 if bs > 16 else 0))
            frames = [spec] * (total // bs) + [dict(assign=assign, sub=dict(kind="VERBATIM"))]
            out[f"bs{bs}_{total}_{bits}"] = (M.stream(x, bits, bs, RATE, frames), x, bits)
    out["lpc32_overflow_24"] = _overflow24() + (24,)
    out["lpc8_overflow_24"] = _overflow24_window() + (24,)
    x = signal(8192 + 5, 2, 24, 9, scale=0.9)                        # the wide cap itself
    out["cap_8192_24"] = (M.stream(x, 24, 8192, RATE, dict(assign=1, sub=dict(kind="VERBATIM"))), x, 24)
    x = signal(16384 + 3, 1, 16, 10)                                  # mono 16-bit keeps its own cap, through the recording entry too
    out["mono16_16384"] = (M.stream(x, 16, 16384, RATE, [dict(sub=dict(kind="FIXED", order=2, porder=4)), dict(sub=dict(kind="VERBATIM"))]), x, 16)
    s, x = verbatim_image()
    out["verbatim_image_16"] = (s, x, 16)
    return out


def above_cap():
    """Stereo 24-bit at block size 8193: refused by the info entry."""
    x = signal(8193 + 2, 2, 24, 11)
    return M.stream(x, 24, 8193, RATE, dict(assign=1, sub=dict(kind="CONSTANT")))


def packing():
    """Five recordings whose PCM lengths make the later ones start at odd bytes: mono-24 of 5 frames (15 bytes), stereo-16, stereo-24
    of 7 frames, mono-16, stereo-24."""
    shapes = ((5, 1, 24), (50, 2, 16), (7, 2, 24), (33, 1, 16), (21, 2, 24))
    out = []
    for i, (n, ch, bits) in enumerate(shapes):
        x = signal(n, ch, bits, 20 + i, scale=0.8)
        out.append((M.stream(x, bits, 16, RATE, dict(sub=dict(kind="FIXED", order=1 if n > 16 else 0))), x, bits))
    return out


def verbatim_image():
    """A stereo-16 stream whose frame 0 carries, byte-aligned inside channel 0's VERBATIM payload, the whole CRC-valid image of its own
    last frame: a candidate the scan finds and the parse accepts, but not on the chain."""
    bs, tail = 64, 17
    x = signal(bs * 2 + tail, 2, 16, 12)
    x[2 * bs:] = (321, -123)
    spec = dict(assign=1, subs=[dict(kind="VERBATIM"), dict(kind="FIXED", order=2)])
    last = dict(assign=1, sub=dict(kind="CONSTANT"))
    image = M.frame([x[2 * bs:, 0].tolist(), x[2 * bs:, 1].tolist()], 2, RATE, 16, last)
    image += b"\0" * (len(image) % 2)
    words = np.frombuffer(image, ">i2").astype(np.int64)
    assert words.size <= bs - 4
    x[4:4 + words.size, 0] = words
    return M.stream(x, 16, bs, RATE, [spec, dict(assign=8), last]), x


@functools.lru_cache(maxsize=None)
def damaged():
    out = {}
    for bits in (16, 24):
        x = signal(64 * 3 + 9, 2, bits, 30 + bits)
        head, frames = M.stream(x, bits, 64, RATE, dict(assign=8), parts=True)
        starts = np.cumsum([len(head)] + [len(f) for f in frames])
        # a bit flip in the side subframe (the frame's second half) of frame 1: CRC-16 no longer holds
        b = bytearray(head + b"".join(frames))
        b[int(starts[1]) + len(frames[1]) - 5] ^= 0x10
        kept = x.copy()
        kept[64:] = 0
        out[f"side_flip_{bits}"] = (bytes(b), "CORRUPT", 1, int(starts[1]), kept, bits)
        # frame 1 coded as a mono frame (valid CRCs): not a frame of a stereo stream
        mono = M.frame([x[64:128, 0].tolist()], 1, RATE, bits, dict(assign=0))
        out[f"mono_frame_{bits}"] = (head + frames[0] + mono + b"".join(frames[2:]), "CORRUPT", 1, int(starts[1]), kept, bits)
        # frame 2, left/side: left at the top of the range, side -1: right = left + 1 is one past it
        full = 1 << (bits - 1)
        bad = M.frame([[0] * 64, [0] * 64], 2, RATE, bits, dict(assign=8, coded=[[full - 1] * 64, [-1] * 64], sub=dict(kind="CONSTANT")))
        kept = x.copy()
        kept[128:192] = 0                                            # (the frame behind it is on the chain and is restored)
        out[f"range_{bits}"] = (head + frames[0] + frames[1] + bad + frames[3], "CORRUPT", 2, int(starts[2]), kept, bits)
        # the same bad frame as frame 1 and a bit flip in frame 3: the chain breaks at frame 3, and the earlier failure is reported
        bad = M.frame([[0] * 64, [0] * 64], 1, RATE, bits, dict(assign=8, coded=[[full - 1] * 64, [-1] * 64], sub=dict(kind="CONSTANT")))
        b = bytearray(head + frames[0] + bad + frames[2] + frames[3])
        b[-5] ^= 0x10
        kept = x.copy()
        kept[64:128] = 0
        kept[192:] = 0
        out[f"range_then_break_{bits}"] = (bytes(b), "CORRUPT", 1, int(starts[1]), kept, bits)
    return out
