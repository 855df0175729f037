"""A FLAC stream writer for the recording decoder's tests: 1 or 2 channels at 16 or 24 bits, a chosen channel assignment per frame
and a spec per subframe, so that a test can reach each branch of a decoder.  From tests/flacmux.py it takes the bit writer, the
residual and Rice-parameter code, the coded number and the metadata blocks; the subframe writer is restated here because the mono
one is fixed at 16 bits.

  stream(samples [frames, channels], bits, bs, rate, frames=None, ...) -> bytes
A frame's spec is a dict (missing keys take the defaults):
  assign      the channel code: 0 (mono), 1 (independent), 8 (left/side), 9 (side/right), 10 (mid/side); default 0 / 1
  sub         one subframe spec for every channel, or subs: one per channel.  A subframe spec is flacmux's: kind, order, coefs,
              precision, shift, porder, ks, method (default: 0 for 16-bit streams, 1 above), wasted
  coded       the channels as they are coded (a list per channel), in place of what the assignment makes of the samples: lets a test
              write a frame whose decorrelated samples leave the depth
  size_code   the header's sample size code (default 4 / 6), number, number_bytes, bs_form: as flacmux
"""
import numpy as np

from flacdec import BLOCK_SIZES, SAMPLE_RATES, crc8, crc16
from flacmux import FIXED, _Bits, _fit_k, block, coded_number, residuals, streaminfo

_BS_CODE = {v: k for k, v in BLOCK_SIZES.items()}
_RATE_CODE = {v: k for k, v in SAMPLE_RATES.items()}


def subframe(b, x, depth, spec):
    """Appends the subframe of the samples x (Python ints) at `depth` bits to the bit writer b."""
    kind, wasted, order = spec.get("kind", "FIXED"), spec.get("wasted", 0), spec.get("order", 0)
    bps = depth - wasted
    if wasted:
        if any(v % (1 << wasted) for v in x):
            raise ValueError("samples are not multiples of 2^wasted")
        x = [v >> wasted for v in x]
    code = {"CONSTANT": 0, "VERBATIM": 1}.get(kind)
    if code is None:
        code = 8 + order if kind == "FIXED" else 31 + order
    b.put(0, 1)
    b.put(code, 6)
    b.put(1 if wasted else 0, 1)
    if wasted:
        b.unary(wasted - 1)
    if kind == "CONSTANT":
        b.put(x[0], bps)
        return
    if kind == "VERBATIM":
        b.parts.append("".join(format(v & ((1 << bps) - 1), f"0{bps}b") for v in x))
        if x and not (-(1 << (bps - 1)) <= min(x) and max(x) < (1 << (bps - 1))):
            raise ValueError("a sample does not fit the subframe's depth")
        return
    for v in x[:order]:
        b.put(v, bps)
    if kind == "LPC":
        coefs, shift, precision = list(spec["coefs"]), spec["shift"], spec["precision"]
        b.put(precision - 1, 4)
        b.put(shift, 5)
        for c in coefs:
            b.put(c, precision)
    else:
        coefs, shift = FIXED[order], 0
    res = residuals(x, coefs, shift)
    method, porder = spec.get("method", 0 if depth <= 17 else 1), spec.get("porder", 0)      # (4-bit parameters stop at 14)
    pbits, esc, kmax = (4, 15, 14) if method == 0 else (5, 31, 30)
    b.put(method, 2)
    b.put(porder, 4)
    n = len(x) >> porder
    ks = spec.get("ks") or [None] * (1 << porder)
    pos = 0
    for p in range(1 << porder):
        count = n - (order if p == 0 else 0)
        part = res[pos:pos + count]
        pos += count
        k = ks[p] if ks[p] is not None else _fit_k(part, kmax)
        if isinstance(k, tuple):
            b.put(esc, pbits)
            b.put(k[1], 5)
            for r in part:
                b.put(r, k[1])
        else:
            b.put(k, pbits)
            out = []
            for r in part:
                u = 2 * r if r >= 0 else -2 * r - 1
                out.append("0" * (u >> k) + "1" + (format(u & ((1 << k) - 1), f"0{k}b") if k else ""))
            b.parts.append("".join(out))


def code_channels(chans, assign):
    """The samples' channels (lists of ints) -> the channels as `assign` codes them."""
    if assign in (0, 1):
        return chans
    left, right = chans
    side = [a - c for a, c in zip(left, right)]
    if assign == 8:
        return [left, side]
    if assign == 9:
        return [side, right]
    return [[(a + c) >> 1 for a, c in zip(left, right)], side]


def frame(chans, index, rate, bits, spec):
    """chans: the frame's samples, a list per channel -> the frame's bytes."""
    bs = len(chans[0])
    assign = spec.get("assign", 0 if len(chans) == 1 else 1)
    form = spec.get("bs_form")
    bs_code = (_BS_CODE.get(bs) or (6 if bs <= 256 else 7)) if form is None else (6 if form == 8 else 7)
    rate_code = _RATE_CODE.get(rate, 0)
    head = bytes([0xFF, 0xF8, (bs_code << 4) | rate_code, (assign << 4) | (spec.get("size_code", 4 if bits == 16 else 6) << 1)])
    head += coded_number(spec.get("number", index), spec.get("number_bytes"))
    if bs_code == 6:
        head += bytes([bs - 1])
    elif bs_code == 7:
        head += (bs - 1).to_bytes(2, "big")
    head += bytes([crc8(head)])
    coded = spec.get("coded") or code_channels(chans, assign)
    subs = spec.get("subs") or [spec.get("sub", dict(kind="FIXED", order=2))] * len(coded)
    b = _Bits()
    for ch, (x, sub) in enumerate(zip(coded, subs)):
        side = (ch == 1 and assign in (8, 10)) or (ch == 0 and assign == 9)
        subframe(b, [int(v) for v in x], bits + (1 if side else 0), sub)
    body = head + b.bytes()
    return body + crc16(body).to_bytes(2, "big")


def stream(samples, bits, bs, rate, frames=None, info=None, parts=False):
    """samples: integers [frames, channels] (or [frames] for mono); frames: one spec per frame, or one for all, or None; info:
    overrides of flacmux.streaminfo()'s arguments.  parts: -> (head, [frame bytes]) instead of the stream."""
    x = np.asarray(samples, np.int64)
    x = x.reshape(-1, 1) if x.ndim == 1 else x
    total, channels = x.shape
    cols = [x[:, c].tolist() for c in range(channels)]
    n_frames = (total + bs - 1) // bs
    if frames is None or isinstance(frames, dict):
        frames = [frames or {}] * n_frames
    out = [frame([c[j * bs:(j + 1) * bs] for c in cols], j, rate, bits, frames[j]) for j in range(n_frames)]
    sizes = [len(f) for f in out]
    kw = dict(bs=bs, rate=rate, total=total, min_frame=min(sizes), max_frame=max(sizes), channels=channels, bits=bits)
    kw.update(info or {})
    head = b"fLaC" + block(0, streaminfo(**kw), last=True)
    return (head, out) if parts else head + b"".join(out)
