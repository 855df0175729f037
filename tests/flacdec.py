"""A FLAC decoder for mono streams of fixed block size, written from RFC 9639 (it shares nothing with tests/flacref.py).  It
rejects rather than guesses: every deviation from the format, and every disagreement between the metadata and the frames, raises
FlacError.

  decode(stream)            -> (int64 samples, info): info has rate, bits, total, min/max block and frame sizes, seek points, frames
"""
import numpy as np


class FlacError(ValueError):
    pass


BLOCK_SIZES = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608, 8: 256, 9: 512, 10: 1024, 11: 2048, 12: 4096, 13: 8192, 14: 16384, 15: 32768}
SAMPLE_RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
SAMPLE_SIZES = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24, 7: 32}


_TABLES = {}


def _crc(data, poly, width):
    top, mask = 1 << (width - 1), (1 << width) - 1
    table = _TABLES.get((poly, width))
    if table is None:
        table = []
        for byte in range(256):
            reg = byte << (width - 8)
            for _ in range(8):
                reg = (reg << 1) ^ (poly if reg & top else 0)
            table.append(reg & mask)
        _TABLES[poly, width] = table
    reg = 0
    for byte in data:
        reg = ((reg << 8) & mask) ^ table[(reg >> (width - 8)) ^ byte]
    return reg


def crc8(data):
    return _crc(data, 0x07, 8)


def crc16(data):
    return _crc(data, 0x8005, 16)


class Bits:
    """A frame as a string of '0' / '1': find() does the unary run in C."""

    def __init__(self, data, start, end):
        self.s = bin(int.from_bytes(b"\x01" + data[start:end], "big"))[3:]
        self.p = 0

    def take(self, n):
        if self.p + n > len(self.s):
            raise FlacError("frame runs past the end of the stream")
        v = int(self.s[self.p:self.p + n], 2) if n else 0
        self.p += n
        return v

    def signed(self, n):
        v = self.take(n)
        return v - (1 << n) if v >> (n - 1) else v

    def unary(self):
        q = self.s.find("1", self.p)
        if q < 0:
            raise FlacError("unary run without its stop bit")
        n = q - self.p
        self.p = q + 1
        return n


def read_coded_number(data, pos):
    if pos >= len(data):
        raise FlacError("truncated frame header")
    b0 = data[pos]
    if b0 < 0x80:
        return b0, 1
    nb = 8 - (b0 ^ 0xFF).bit_length()                    # leading ones
    if nb < 2 or nb > 7:
        raise FlacError("bad coded number")
    if pos + nb > len(data):
        raise FlacError("truncated frame header")
    v = b0 & ((1 << (7 - nb)) - 1) if nb < 7 else 0
    for j in range(1, nb):
        if data[pos + j] & 0xC0 != 0x80:
            raise FlacError("bad continuation byte in a coded number")
        v = (v << 6) | (data[pos + j] & 0x3F)
    return v, nb


def read_residual(bits, bs, order, out):
    method = bits.take(2)
    if method > 1:
        raise FlacError("reserved residual coding method")
    pbits, esc = (4, 15) if method == 0 else (5, 31)
    porder = bits.take(4)
    if bs % (1 << porder) or (bs >> porder) < order:
        raise FlacError("partition order does not fit the block")
    ks = []
    for p in range(1 << porder):
        count = (bs >> porder) - (order if p == 0 else 0)
        if count < 0:
            raise FlacError("partition shorter than the predictor order")
        k = bits.take(pbits)
        ks.append(k)
        if k == esc:
            w = bits.take(5)
            for _ in range(count):
                out.append(bits.signed(w) if w else 0)
        else:
            for _ in range(count):
                u = (bits.unary() << k) | bits.take(k)
                out.append((u >> 1) ^ -(u & 1))
    return method, porder, ks


def read_subframe(bits, bs, bps):
    if bits.take(1):
        raise FlacError("subframe padding bit set")
    kind = bits.take(6)
    if bits.take(1):
        wasted = bits.unary() + 1
    else:
        wasted = 0
    bps -= wasted
    meta = dict(wasted=wasted)
    if kind == 0:
        x = np.full(bs, bits.signed(bps), np.int64)
        meta.update(kind="CONSTANT")
    elif kind == 1:
        x = [bits.signed(bps) for _ in range(bs)]
        meta.update(kind="VERBATIM")
    elif 8 <= kind <= 12:
        order = kind - 8
        if order > bs:
            raise FlacError("predictor order above the block size")
        x = [bits.signed(bps) for _ in range(order)]
        res = []
        method, porder, ks = read_residual(bits, bs, order, res)
        coef = [[], [1], [2, -1], [3, -3, 1], [4, -6, 4, -1]][order]
        for r in res:
            x.append(r + sum(c * x[-1 - j] for j, c in enumerate(coef)))
        meta.update(kind="FIXED", order=order, porder=porder, ks=ks, method=method)
    else:
        raise FlacError(f"subframe type {kind} is reserved or not handled (LPC)")
    x = np.asarray(x, np.int64)
    return (x << wasted if wasted else x), meta


def read_frame(data, pos, info):
    """-> (samples, meta, the frame's end)"""
    if pos + 6 > len(data):
        raise FlacError("truncated frame")
    if data[pos] != 0xFF or data[pos + 1] & 0xFC != 0xF8:
        raise FlacError("bad frame sync")
    if data[pos + 1] & 0x02:
        raise FlacError("reserved bit after the sync is set")
    variable = data[pos + 1] & 1
    bs_code, rate_code = data[pos + 2] >> 4, data[pos + 2] & 15
    channels, size_code, reserved = data[pos + 3] >> 4, (data[pos + 3] >> 1) & 7, data[pos + 3] & 1
    if reserved:
        raise FlacError("reserved bit in the frame header is set")
    if bs_code == 0 or rate_code == 15 or size_code == 3:
        raise FlacError("reserved code in the frame header")
    if channels != 0:
        raise FlacError("only mono is handled")
    number, nb = read_coded_number(data, pos + 4)
    p = pos + 4 + nb
    if bs_code == 6:
        bs, p = data[p] + 1, p + 1
    elif bs_code == 7:
        bs, p = ((data[p] << 8) | data[p + 1]) + 1, p + 2
    else:
        bs = BLOCK_SIZES[bs_code]
    if rate_code == 0:
        rate = info["rate"]
    elif rate_code == 12:
        rate, p = data[p] * 1000, p + 1
    elif rate_code == 13:
        rate, p = (data[p] << 8) | data[p + 1], p + 2
    elif rate_code == 14:
        rate, p = ((data[p] << 8) | data[p + 1]) * 10, p + 2
    else:
        rate = SAMPLE_RATES[rate_code]
    bps = info["bits"] if size_code == 0 else SAMPLE_SIZES[size_code]
    if rate != info["rate"] or bps != info["bits"]:
        raise FlacError("frame header disagrees with STREAMINFO")
    if crc8(data[pos:p]) != data[p]:
        raise FlacError("wrong CRC-8")
    p += 1
    bits = Bits(data, p, pos + info["max_frame"] if info["max_frame"] else len(data))      # (0 = unknown)
    x, meta = read_subframe(bits, bs, bps)
    pad = (-bits.p) % 8
    if bits.take(pad):
        raise FlacError("non-zero padding")
    end = p + bits.p // 8
    if end + 2 > len(data):
        raise FlacError("truncated frame")
    if crc16(data[pos:end]) != (data[end] << 8) | data[end + 1]:
        raise FlacError("wrong CRC-16")
    meta.update(number=number, number_bytes=nb, variable=variable, bs=bs, bs_code=bs_code, rate_code=rate_code, start=pos, bytes=end + 2 - pos)
    return x, meta, end + 2


def decode(stream):
    data = bytes(stream)
    if data[:4] != b"fLaC":
        raise FlacError("no fLaC marker")
    pos, last, info, first = 4, False, None, True
    seek = []
    while not last:
        if pos + 4 > len(data):
            raise FlacError("truncated metadata")
        last, kind = bool(data[pos] & 0x80), data[pos] & 0x7F
        size = int.from_bytes(data[pos + 1:pos + 4], "big")
        body = data[pos + 4:pos + 4 + size]
        if len(body) != size:
            raise FlacError("truncated metadata block")
        if first != (kind == 0):
            raise FlacError("STREAMINFO must be the first block, once")
        if kind == 0:
            if size != 34:
                raise FlacError("STREAMINFO is 34 bytes")
            v = int.from_bytes(body[10:18], "big")
            info = dict(min_block=int.from_bytes(body[0:2], "big"), max_block=int.from_bytes(body[2:4], "big"),
                        min_frame=int.from_bytes(body[4:7], "big"), max_frame=int.from_bytes(body[7:10], "big"),
                        rate=v >> 44, channels=((v >> 41) & 7) + 1, bits=((v >> 36) & 31) + 1, total=v & ((1 << 36) - 1), md5=body[18:34])
            if info["channels"] != 1:
                raise FlacError("only mono is handled")
            if info["min_block"] < 16 or info["min_block"] > info["max_block"]:
                raise FlacError("bad block size bounds")
        elif kind == 3:
            if size % 18:
                raise FlacError("SEEKTABLE is a whole number of points")
            seek = [(int.from_bytes(body[i:i + 8], "big"), int.from_bytes(body[i + 8:i + 16], "big"), int.from_bytes(body[i + 16:i + 18], "big"))
                    for i in range(0, size, 18)]
        elif kind == 127:
            raise FlacError("forbidden metadata block type")
        first = False
        pos += 4 + size
    audio = pos
    samples, frames, count = [], [], 0
    while pos < len(data):
        x, meta, pos = read_frame(data, pos, info)
        if meta["variable"]:
            raise FlacError("variable block size streams are not handled")
        if meta["number"] != len(frames):
            raise FlacError("frame numbers are not consecutive")
        if frames and frames[-1]["bs"] != info["max_block"]:
            raise FlacError("only the last frame may be short")
        if meta["bs"] > info["max_block"]:
            raise FlacError("block larger than STREAMINFO's maximum")
        meta["first_sample"] = count
        count += x.size
        samples.append(x)
        frames.append(meta)
    if count != info["total"]:
        raise FlacError(f"decoded {count} samples, STREAMINFO says {info['total']}")
    sizes = [m["bytes"] for m in frames]
    if sizes and (info["min_frame"] != min(sizes) or info["max_frame"] != max(sizes)):
        raise FlacError("STREAMINFO's frame sizes disagree with the frames")
    starts = {m["start"] - audio: m for m in frames}
    prev = -1
    for sample, offset, count in seek:
        m = starts.get(offset)
        if m is None or m["first_sample"] != sample or m["bs"] != count:
            raise FlacError("seek point does not land on the named frame's header")
        if sample <= prev:
            raise FlacError("seek points must ascend")
        prev = sample
    lim = 1 << (info["bits"] - 1)
    out = np.concatenate(samples) if samples else np.zeros(0, np.int64)
    if out.size and (out.min() < -lim or out.max() >= lim):
        raise FlacError("sample outside the stream's bit depth")
    info.update(seek=seek, frames=frames)
    return out, info
