"""A FLAC decoder for recordings, restated from RFC 9639 on its own (it shares no code with tests/flacdec.py, tests/flaclpcdec.py
or birdnet-go_amd/csrc/flac_parse.h): streams of 1 or 2 channels at 16 or 24 bits and a fixed block size, every subframe kind,
both residual coding methods, the four stereo channel assignments.  It works on Python integers, so nothing can overflow, and it
refuses rather than guesses: any deviation raises WideFlacError.

  decode(stream)  -> (int64 samples [frames, channels], info): info has rate, bits, channels, total, block, audio (the first
                     frame's offset) and frames: per frame start, size, number, block, assign and per subframe kind / order / wasted /
                     method / porder / escapes (the partitions that are escape-coded)
  pcm_bytes(x, bits) -> the interleaved little-endian PCM of such samples: what a WAV data chunk of the audio holds
"""
import numpy as np


class WideFlacError(ValueError):
    pass


_BLOCK = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608}
_RATE = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
_DEPTH = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}
_FIXED = ((), (1,), (2, -1), (3, -3, 1), (4, -6, 4, -1))


def _crc(data, poly, width):
    reg, top, mask = 0, 1 << (width - 1), (1 << width) - 1
    for byte in data:
        reg ^= byte << (width - 8)
        for _ in range(8):
            reg = ((reg << 1) ^ poly) & mask if reg & top else (reg << 1) & mask
    return reg


class _Reader:
    """The bits of data[start:] as one big integer, most significant first."""

    def __init__(self, data, start):
        self.total = 8 * (len(data) - start)
        self.text = format(int.from_bytes(data[start:], "big"), f"0{self.total}b") if self.total else ""
        self.at = 0

    def u(self, n):
        if n == 0:
            return 0
        if self.at + n > self.total:
            raise WideFlacError("the frame runs past the end of the stream")
        v = int(self.text[self.at:self.at + n], 2)
        self.at += n
        return v

    def s(self, n):
        v = self.u(n)
        return v - (1 << n) if v >= 1 << (n - 1) else v

    def zeros(self):
        stop = self.text.find("1", self.at)
        if stop < 0:
            raise WideFlacError("a unary run without its stop bit")
        n, self.at = stop - self.at, stop + 1
        return n


def _residual(rd, block, order):
    method = rd.u(2)
    if method > 1:
        raise WideFlacError("reserved residual coding method")
    width, escape = (4, 15) if method == 0 else (5, 31)
    porder = rd.u(4)
    parts = 1 << porder
    if block % parts or block // parts < order:
        raise WideFlacError("the partition order does not fit the block")
    out, escapes = [], 0
    for part in range(parts):
        n = block // parts - (order if part == 0 else 0)
        k = rd.u(width)
        if k == escape:
            escapes += 1
            raw = rd.u(5)
            out.extend(rd.s(raw) if raw else 0 for _ in range(n))
        else:
            for _ in range(n):
                folded = (rd.zeros() << k) | rd.u(k)
                out.append(-(folded >> 1) - 1 if folded & 1 else folded >> 1)
    return out, dict(method=method, porder=porder, escapes=escapes)


def _subframe(rd, block, depth):
    if rd.u(1):
        raise WideFlacError("the subframe's padding bit is set")
    code = rd.u(6)
    wasted = rd.zeros() + 1 if rd.u(1) else 0
    if wasted >= depth:
        raise WideFlacError("more wasted bits than the subframe has")
    depth -= wasted
    lo, hi = -(1 << (depth - 1)), (1 << (depth - 1)) - 1
    meta = dict(wasted=wasted)
    if code == 0:
        x = [rd.s(depth)] * block
        meta.update(kind="CONSTANT")
    elif code == 1:
        x = [rd.s(depth) for _ in range(block)]
        meta.update(kind="VERBATIM")
    elif 8 <= code <= 12 or code >= 32:
        order = code - 8 if code < 32 else code - 31
        if order > block:
            raise WideFlacError("the predictor's order is above the block size")
        x = [rd.s(depth) for _ in range(order)]
        if code >= 32:
            precision = rd.u(4) + 1
            if precision == 16:
                raise WideFlacError("reserved coefficient precision")
            shift = rd.s(5)
            if shift < 0:
                raise WideFlacError("negative predictor shift")
            coefs = [rd.s(precision) for _ in range(order)]
            meta.update(kind="LPC", precision=precision, shift=shift)
        else:
            coefs, shift = list(_FIXED[order]), 0
            meta.update(kind="FIXED")
        res, coding = _residual(rd, block, order)
        meta.update(coding, order=order)
        for r in res:
            acc = 0
            for j in range(order):
                acc += coefs[j] * x[-1 - j]
            v = r + (acc >> shift)
            if v < lo or v > hi:
                raise WideFlacError("a predicted sample leaves the subframe's depth")
            x.append(v)
    else:
        raise WideFlacError(f"reserved subframe type {code}")
    return [v << wasted for v in x], meta


def _number(data, at):
    first = data[at]
    if first < 0x80:
        return first, 1
    n = 0
    while n < 8 and first & (0x80 >> n):
        n += 1
    if n < 2 or n > 7 or at + n > len(data):
        raise WideFlacError("bad coded number")
    v = first & ((1 << (7 - n)) - 1) if n < 7 else 0
    for b in data[at + 1:at + n]:
        if b >> 6 != 2:
            raise WideFlacError("bad continuation byte")
        v = (v << 6) | (b & 63)
    return v, n


def _frame(data, at, info):
    if at + 6 > len(data) or data[at] != 0xFF or data[at + 1] != 0xF8:
        raise WideFlacError("no fixed-block-size frame sync")
    bcode, rcode = data[at + 2] >> 4, data[at + 2] & 15
    assign, dcode = data[at + 3] >> 4, (data[at + 3] >> 1) & 7
    if data[at + 3] & 1 or bcode == 0 or rcode == 15 or dcode == 3:
        raise WideFlacError("reserved header value")
    channels = assign + 1 if assign < 8 else 2
    if assign > 10 or channels != info["channels"]:
        raise WideFlacError("the frame's channels disagree with STREAMINFO")
    number, used = _number(data, at + 4)
    p = at + 4 + used
    if bcode == 6:
        block, p = data[p] + 1, p + 1
    elif bcode == 7:
        block, p = int.from_bytes(data[p:p + 2], "big") + 1, p + 2
    else:
        block = _BLOCK[bcode] if bcode < 6 else 256 << (bcode - 8)
    if rcode == 0:
        rate = info["rate"]
    elif rcode == 12:
        rate, p = data[p] * 1000, p + 1
    elif rcode == 13:
        rate, p = int.from_bytes(data[p:p + 2], "big"), p + 2
    elif rcode == 14:
        rate, p = int.from_bytes(data[p:p + 2], "big") * 10, p + 2
    else:
        rate = _RATE[rcode]
    depth = info["bits"] if dcode == 0 else _DEPTH[dcode]
    if rate != info["rate"] or depth != info["bits"]:
        raise WideFlacError("the frame's rate or depth disagrees with STREAMINFO")
    if _crc(data[at:p], 0x07, 8) != data[p]:
        raise WideFlacError("wrong CRC-8")
    rd = _Reader(data, p + 1)
    coded, subs = [], []
    for ch in range(channels):
        side = (ch == 1 and assign in (8, 10)) or (ch == 0 and assign == 9)
        x, meta = _subframe(rd, block, depth + (1 if side else 0))
        coded.append(x)
        subs.append(meta)
    if rd.u((-rd.at) % 8):
        raise WideFlacError("non-zero padding")
    end = p + 1 + rd.at // 8
    if end + 2 > len(data) or _crc(data[at:end], 0x8005, 16) != int.from_bytes(data[end:end + 2], "big"):
        raise WideFlacError("wrong CRC-16")
    if assign == 8:
        left, right = coded[0], [a - s for a, s in zip(coded[0], coded[1])]
    elif assign == 9:
        left, right = [s + r for s, r in zip(coded[0], coded[1])], coded[1]
    elif assign == 10:
        left, right = [], []
        for mid, s in zip(coded[0], coded[1]):
            mid = (mid << 1) | (s & 1)
            left.append((mid + s) >> 1)
            right.append((mid - s) >> 1)
    else:
        left, right = coded[0], coded[-1]
    out = [left, right][:channels]
    lo, hi = -(1 << (depth - 1)), (1 << (depth - 1)) - 1
    if any(v < lo or v > hi for ch in out for v in ch):
        raise WideFlacError("a decorrelated sample leaves the stream's depth")
    return out, dict(start=at, size=end + 2 - at, number=number, block=block, assign=assign, subframes=subs), end + 2


def metadata(stream):
    """The marker and metadata blocks alone -> info (without frames)."""
    data = bytes(stream)
    if data[:4] != b"fLaC":
        raise WideFlacError("no fLaC marker")
    at, info, index, seek = 4, None, 0, 0
    while True:
        if at + 4 > len(data):
            raise WideFlacError("truncated metadata")
        last, kind, size = data[at] >> 7, data[at] & 127, int.from_bytes(data[at + 1:at + 4], "big")
        body = data[at + 4:at + 4 + size]
        if len(body) != size or kind == 127 or (index == 0) != (kind == 0):
            raise WideFlacError("bad metadata block")
        if kind == 0:
            if size != 34:
                raise WideFlacError("STREAMINFO holds 34 bytes")
            packed = int.from_bytes(body[10:18], "big")
            info = dict(min_block=int.from_bytes(body[0:2], "big"), block=int.from_bytes(body[2:4], "big"),
                        min_frame=int.from_bytes(body[4:7], "big"), max_frame=int.from_bytes(body[7:10], "big"), rate=packed >> 44,
                        channels=((packed >> 41) & 7) + 1, bits=((packed >> 36) & 31) + 1, total=packed & ((1 << 36) - 1))
            if info["min_block"] < 16 or info["min_block"] > info["block"]:
                raise WideFlacError("bad block size bounds")
        elif kind == 3:
            seek = size // 18
        at += 4 + size
        index += 1
        if last:
            break
    info.update(audio=at, seek_points=seek)
    return info


def decode(stream):
    data = bytes(stream)
    info = metadata(data)
    if info["channels"] > 2 or info["bits"] not in (16, 24):
        raise WideFlacError("only 1 or 2 channels at 16 or 24 bits are handled")
    at, frames, chans, done = info["audio"], [], [[] for _ in range(info["channels"])], 0
    while at < len(data):
        out, meta, at = _frame(data, at, info)
        if meta["number"] != len(frames):
            raise WideFlacError("frame numbers are not consecutive")
        want = min(info["block"], info["total"] - done)
        if meta["block"] != want:
            raise WideFlacError("a frame's block size is not the one its place in the stream demands")
        for ch, x in zip(chans, out):
            ch.extend(x)
        done += meta["block"]
        frames.append(meta)
    if done != info["total"]:
        raise WideFlacError("the frames do not hold STREAMINFO's sample count")
    info["frames"] = frames
    return np.array(chans, np.int64).T.reshape(done, info["channels"]), info


def pcm_bytes(x, bits):
    x = np.asarray(x, np.int64).reshape(-1)
    if bits == 16:
        return x.astype("<i2").tobytes()
    u = (x & 0xFFFFFF).astype(np.uint32)
    return np.stack([u & 255, (u >> 8) & 255, (u >> 16) & 255], axis=1).astype(np.uint8).tobytes()
