"""A FLAC decoder for mono streams of fixed block size whose frames may hold LPC subframes, written from RFC 9639 (§9.2.6 for the
LPC subframe).  It shares nothing with tests/flaclpcref.py.  From tests/flacdec.py it takes the bit reader, the CRCs, the coded
number and the residual reader; the subframes and the walk over metadata and frames are stated here.  It rejects what flacdec
rejects, and besides a coefficient precision of `1111` and a negative shift.

  decode(stream)            -> (int64 samples, info): info as flacdec's; an LPC frame's meta has order, precision, shift, coefs
"""
import numpy as np

from flacdec import BLOCK_SIZES, SAMPLE_RATES, SAMPLE_SIZES, Bits, FlacError, crc8, crc16, read_coded_number, read_residual

FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


def read_subframe(bits, bs, bps):
    if bits.take(1):
        raise FlacError("subframe padding bit set")
    kind = bits.take(6)
    wasted = bits.unary() + 1 if bits.take(1) else 0
    bps -= wasted
    if bps < 1:
        raise FlacError("more wasted bits than sample bits")
    meta = dict(wasted=wasted)
    if kind == 0:
        x = [bits.signed(bps)] * bs
        meta.update(kind="CONSTANT")
    elif kind == 1:
        x = [bits.signed(bps) for _ in range(bs)]
        meta.update(kind="VERBATIM")
    elif 8 <= kind <= 12 or kind >= 32:
        order = kind - 8 if kind < 32 else kind - 31
        if order > bs:
            raise FlacError("predictor order above the block size")
        x = [bits.signed(bps) for _ in range(order)]
        if kind < 32:
            coefs, shift = FIXED[order], 0
            meta.update(kind="FIXED", order=order)
        else:
            precision = bits.take(4) + 1
            if precision == 16:
                raise FlacError("coefficient precision 1111 is forbidden")
            shift = bits.signed(5)
            if shift < 0:
                raise FlacError("negative prediction shift")
            coefs = [bits.signed(precision) for _ in range(order)]
            meta.update(kind="LPC", order=order, precision=precision, shift=shift, coefs=coefs)
        res = []
        method, porder, ks = read_residual(bits, bs, order, res)
        if len(res) != bs - order:
            raise FlacError("residual count does not fill the block")
        for r in res:
            pred = 0
            for j, c in enumerate(coefs):
                pred += c * x[-1 - j]
            x.append(r + (pred >> shift))
        meta.update(porder=porder, ks=ks, method=method)
    else:
        raise FlacError(f"subframe type {kind} is reserved")
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
    extra = (1 if bs_code == 6 else 2 if bs_code == 7 else 0) + (1 if rate_code == 12 else 2 if rate_code in (13, 14) else 0)
    if p + extra + 1 > len(data):
        raise FlacError("truncated frame header")
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
    if bits.take((-bits.p) % 8):
        raise FlacError("non-zero padding")
    end = p + bits.p // 8
    if end + 2 > len(data):
        raise FlacError("truncated frame")
    if crc16(data[pos:end]) != (data[end] << 8) | data[end + 1]:
        raise FlacError("wrong CRC-16")
    meta.update(number=number, number_bytes=nb, variable=variable, bs=bs, bs_code=bs_code, rate_code=rate_code, start=pos, bytes=end + 2 - pos)
    return x, meta, end + 2


def read_metadata(data):
    """-> (STREAMINFO's fields, the seek points, where the frames begin)"""
    if data[:4] != b"fLaC":
        raise FlacError("no fLaC marker")
    pos, last, info, seek, blocks = 4, False, None, [], 0
    while not last:
        if pos + 4 > len(data):
            raise FlacError("truncated metadata")
        last, kind = bool(data[pos] & 0x80), data[pos] & 0x7F
        size = int.from_bytes(data[pos + 1:pos + 4], "big")
        body = data[pos + 4:pos + 4 + size]
        if len(body) != size:
            raise FlacError("truncated metadata block")
        if (blocks == 0) != (kind == 0):
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
        blocks += 1
        pos += 4 + size
    return info, seek, pos


def decode(stream):
    data = bytes(stream)
    info, seek, audio = read_metadata(data)
    pos, samples, frames, count = audio, [], [], 0
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
    for sample, offset, length in seek:
        m = starts.get(offset)
        if m is None or m["first_sample"] != sample or m["bs"] != length:
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
