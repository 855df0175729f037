"""A FLAC stream writer for the decoder's tests, written from RFC 9639: mono streams of fixed block size whose every frame takes
explicit choices, so that a test can reach each branch of a decoder.  It computes the residuals from the samples, so every stream it
writes is valid unless a test asks otherwise.  It shares nothing with tests/flacref.py; from tests/flacdec.py it takes the CRCs and
the code tables.

  stream(samples, bs, rate, frames=None, ...) -> bytes
A frame's spec is a dict (missing keys take the defaults):
  kind        "CONSTANT", "VERBATIM", "FIXED" (order 0..4) or "LPC" (order 1..32 with coefs, precision 1..15, shift 0..15)
  order, coefs, precision, shift
  porder      partition order; ks: per partition a Rice parameter, or ("esc", width); None: a fitting parameter per partition
  method      0 (4-bit parameters, escape 15) or 1 (5-bit, escape 31)
  wasted      wasted bits (the samples must be multiples of 2^wasted)
  bs_form     None (a table code where there is one), 8 or 16: the explicit forms
  rate_form   None (a table code where there is one, else "as STREAMINFO"), 0, 12, 13 or 14
  number      the coded number (default: the frame's index); number_bytes: its coded length (default: the shortest)
  variable    the blocking-strategy bit
"""
import numpy as np

from flacdec import BLOCK_SIZES, SAMPLE_RATES, crc8, crc16

FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}
_BS_CODE = {v: k for k, v in BLOCK_SIZES.items()}
_RATE_CODE = {v: k for k, v in SAMPLE_RATES.items()}


class _Bits:
    def __init__(self):
        self.parts = []

    def put(self, v, n):
        if n:
            v = int(v)
            if not -(1 << (n - 1)) <= v < (1 << n):
                raise ValueError(f"{v} does not fit {n} bits")
            self.parts.append(format(v & ((1 << n) - 1), f"0{n}b"))

    def unary(self, q):
        self.parts.append("0" * int(q) + "1")

    def bytes(self):
        s = "".join(self.parts)
        s += "0" * ((-len(s)) % 8)
        return int(s, 2).to_bytes(len(s) // 8, "big") if s else b""


def coded_number(v, nbytes=None):
    need = 1 if v < 0x80 else next(n for n in range(2, 8) if v < 1 << (5 * n + 1))
    n = nbytes or need
    if n < need:
        raise ValueError("number does not fit")
    if n == 1:
        return bytes([v])
    lead = (0xFF << (8 - n)) & 0xFF
    out = [lead | (v >> (6 * (n - 1)) if n < 7 else 0)]
    for j in range(n - 2, -1, -1):
        out.append(0x80 | ((v >> (6 * j)) & 0x3F))
    return bytes(out)


def residuals(x, coefs, shift):
    order = len(coefs)
    res = []
    for i in range(order, len(x)):
        pred = sum(c * x[i - 1 - j] for j, c in enumerate(coefs))
        res.append(x[i] - (pred >> shift))
    return res


def _fit_k(part, kmax):
    mean = sum(2 * r if r >= 0 else -2 * r - 1 for r in part) / max(len(part), 1)
    return min(max(int(mean).bit_length() - 1, 0), kmax)


def subframe(x, spec):
    """x: the frame's samples as Python ints -> the subframe's bit writer."""
    b = _Bits()
    kind = spec.get("kind", "FIXED")
    wasted = spec.get("wasted", 0)
    bps = 16 - wasted
    if wasted:
        if any(v % (1 << wasted) for v in x):
            raise ValueError("samples are not multiples of 2^wasted")
        x = [v >> wasted for v in x]
    order = spec.get("order", 0)
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
        return b
    if kind == "VERBATIM":
        for v in x:
            b.put(v, bps)
        return b
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
    method, porder = spec.get("method", 0), spec.get("porder", 0)
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
                if k[1]:
                    if not -(1 << (k[1] - 1)) <= r < (1 << (k[1] - 1)):
                        raise ValueError("residual does not fit the escape width")
                    b.put(r, k[1])
                elif r:
                    raise ValueError("a width-0 partition holds a non-zero residual")
        else:
            b.put(k, pbits)
            for r in part:
                u = 2 * r if r >= 0 else -2 * r - 1
                b.unary(u >> k)
                b.put(u & ((1 << k) - 1), k)
    return b


def frame(x, index, rate, spec):
    bs = len(x)
    form = spec.get("bs_form")
    if form is None:
        bs_code = _BS_CODE.get(bs) or (6 if bs <= 256 else 7)
    else:
        bs_code = 6 if form == 8 else 7
    rform = spec.get("rate_form")
    rate_code = rform if rform is not None else _RATE_CODE.get(rate, 0)
    head = bytes([0xFF, 0xF8 | (1 if spec.get("variable") else 0), (bs_code << 4) | rate_code, spec.get("size_code", 4) << 1])
    head += coded_number(spec.get("number", index), spec.get("number_bytes"))
    if bs_code == 6:
        head += bytes([bs - 1])
    elif bs_code == 7:
        head += (bs - 1).to_bytes(2, "big")
    if rate_code == 12:
        head += bytes([rate // 1000])
    elif rate_code == 13:
        head += rate.to_bytes(2, "big")
    elif rate_code == 14:
        head += (rate // 10).to_bytes(2, "big")
    head += bytes([crc8(head)])
    body = head + subframe([int(v) for v in x], spec).bytes()
    return body + crc16(body).to_bytes(2, "big")


def streaminfo(bs, rate, total, min_frame, max_frame, channels=1, bits=16, min_block=None):
    v = (rate << 44) | ((channels - 1) << 41) | ((bits - 1) << 36) | total
    return ((bs if min_block is None else min_block).to_bytes(2, "big") + bs.to_bytes(2, "big") + min_frame.to_bytes(3, "big") +
            max_frame.to_bytes(3, "big") + v.to_bytes(8, "big") + bytes(16))


def block(kind, body, last=False):
    return bytes([(0x80 if last else 0) | kind]) + len(body).to_bytes(3, "big") + body


def stream(samples, bs, rate, frames=None, blocks=(), info=None, parts=False):
    """samples: integers (int16 range unless a test wants otherwise); frames: one spec per frame, or one for all, or None (FIXED order 2);
    blocks: extra (kind, body) metadata blocks after STREAMINFO; info: overrides of streaminfo()'s arguments.  parts: -> (head, [frame
    bytes]) instead of the stream."""
    x = [int(v) for v in np.asarray(samples).reshape(-1)]
    n_frames = (len(x) + bs - 1) // bs
    if frames is None or isinstance(frames, dict):
        frames = [frames or dict(kind="FIXED", order=2)] * n_frames
    out = [frame(x[j * bs:(j + 1) * bs], j, rate, frames[j]) for j in range(n_frames)]
    sizes = [len(f) for f in out]
    kw = dict(bs=bs, rate=rate, total=len(x), min_frame=min(sizes), max_frame=max(sizes))
    kw.update(info or {})
    head = b"fLaC" + block(0, streaminfo(**kw), last=not blocks)
    for i, (kind, body) in enumerate(blocks):
        head += block(kind, body, last=i == len(blocks) - 1)
    return (head, out) if parts else head + b"".join(out)
