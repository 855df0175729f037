"""The FLAC encoder spec of DESIGN.md §9 restated in numpy: the analysis vectorised over a clip's frames, the bits of a frame laid
out from (position, length, value) fields.  Integers only, so the device's bytes must equal these.

  encode(x, rate, seek_interval=0)            -> the stream's bytes
  encode(x, rate, seek_interval, info=True)   -> (bytes, [one dict per frame: kind, order, porder, ks, bs, bits, bytes, ...])
  encode_batch(clips, rate, factor, seek)     -> (all streams back to back, offsets uint64 [B + 1]), the gain of loudref applied
"""
import numpy as np

import loudref

BLOCK = 4096
RATES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
FIXED_COEF = [[1], [1, -1], [1, -2, 1], [1, -3, 3, -1], [1, -4, 6, -4, 1]]


def _crc_table(poly, width):
    top, mask = 1 << (width - 1), (1 << width) - 1
    t = []
    for b in range(256):
        c = b << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        t.append(c)
    return t


_T8, _T16 = _crc_table(0x07, 8), _crc_table(0x8005, 16)
_M16 = None            # _M16[d][b] = b x^(8 d + 16) mod P: the CRC-16 is linear, so a message's is the XOR of its bytes' rows


def crc8(data):
    c = 0
    for b in data:
        c = _T8[c ^ b]
    return c


def crc16(data):
    global _M16
    a = np.frombuffer(bytes(data), np.uint8)
    if _M16 is None or _M16.shape[0] < a.size:
        rows = max(a.size, 8300)
        t = np.array(_T16, np.uint16)
        m = np.empty((rows, 256), np.uint16)
        m[0] = t
        for d in range(1, rows):
            m[d] = (m[d - 1] << np.uint16(8)) ^ t[m[d - 1] >> np.uint16(8)]
        _M16 = m
    if a.size == 0:
        return 0
    return int(np.bitwise_xor.reduce(_M16[a.size - 1 - np.arange(a.size), a]))


def coded_number(v):
    """The UTF-8-style coding of a frame number: 1 to 7 bytes."""
    if v < 0x80:
        return bytes([v])
    nb = next(i for i, lim in zip(range(2, 8), (1 << 11, 1 << 16, 1 << 21, 1 << 26, 1 << 31, 1 << 36)) if v < lim)
    out = [((0xFF00 >> nb) & 0xFF) | (v >> (6 * (nb - 1)))]
    out += [0x80 | ((v >> (6 * j)) & 0x3F) for j in range(nb - 2, -1, -1)]
    return bytes(out)


def frame_header(frame_no, bs, rate):
    code = 12 if bs == BLOCK else 6 if bs <= 256 else 7
    h = bytes([0xFF, 0xF8, (code << 4) | RATES.get(rate, 0), 0x08]) + coded_number(frame_no)
    if code == 6:
        h += bytes([bs - 1])
    elif code == 7:
        h += bytes([(bs - 1) >> 8, (bs - 1) & 0xFF])
    return h + bytes([crc8(h)])


def analyse(frames):
    """frames int64 [F, bs], none of them constant -> per frame (fixed bits, order, porder, ks [F][..]): the exact minimum over
    o, P and k; ties to the lowest k, then the lowest P, then the lowest o."""
    F, bs = frames.shape
    tz = (bs & -bs).bit_length() - 1
    pmax, omax = min(5, tz), min(4, bs - 1)
    best_bits = np.full(F, np.iinfo(np.int64).max, np.int64)
    best_o, best_p = np.zeros(F, np.int64), np.zeros(F, np.int64)
    best_k = np.zeros((F, 32), np.int64)
    table = {}
    for o in range(omax + 1):
        r = np.zeros((F, bs), np.int64)
        for j, c in enumerate(FIXED_COEF[o]):
            r[:, o:] += c * frames[:, o - j:bs - j]
        u = np.where(r >= 0, 2 * r, -2 * r - 1)
        u[:, :o] = 0                                            # the warm-up samples have no residual
        fine = np.stack([(u >> k).reshape(F, 1 << pmax, -1).sum(2) for k in range(15)], 2)       # [F, parts, 15]
        for P in range(pmax, -1, -1):
            if P < pmax:
                fine = fine[:, 0::2] + fine[:, 1::2]            # sums of pairs: exact
            if (bs >> P) <= o:
                continue
            cnt = np.full(1 << P, bs >> P, np.int64)
            cnt[0] -= o
            bits = (1 + np.arange(15))[None, None, :] * cnt[None, :, None] + fine
            ks = bits.argmin(2)                                 # (the first minimum: the lowest k)
            table[o, P] = (8 + 16 * o + 6 + (4 + bits.min(2)).sum(1), ks)
    for P in range(pmax + 1):
        for o in range(omax + 1):
            if (o, P) not in table:
                continue
            cost, ks = table[o, P]
            win = cost < best_bits
            best_bits[win], best_o[win], best_p[win] = cost[win], o, P
            best_k[win, :1 << P] = ks[win]
    return best_bits, best_o, best_p, best_k


def pack_fields(pos, length, val, total_bits):
    """ORs `length` low bits of `val` at bit `pos` (MSB first) for every field; -> bytes, zero-padded to a byte."""
    bits = np.zeros(((total_bits + 7) // 8) * 8, np.uint8)
    pos, length, val = (np.asarray(a, np.int64) for a in (pos, length, val))
    for j in range(int(length.max()) if length.size else 0):
        m = length > j
        bits[pos[m] + j] = (val[m] >> (length[m] - 1 - j)) & 1
    return np.packbits(bits).tobytes()


def subframe(x, kind, o=0, P=0, ks=None):
    """-> (bytes, bits) of one subframe of the int64 block x."""
    bs = x.size
    if kind == "CONSTANT":
        return pack_fields([0, 8], [8, 16], [0x00, int(x[0]) & 0xFFFF], 24), 24
    if kind == "VERBATIM":
        pos = np.concatenate([[0], 8 + 16 * np.arange(bs)])
        return pack_fields(pos, np.concatenate([[8], np.full(bs, 16)]), np.concatenate([[0x02], x & 0xFFFF]), 8 + 16 * bs), 8 + 16 * bs
    r = np.zeros(bs, np.int64)
    for j, c in enumerate(FIXED_COEF[o]):
        r[o:] += c * x[o - j:bs - j]
    u = np.where(r >= 0, 2 * r, -2 * r - 1)[o:]
    idx = np.arange(o, bs)
    lp = bs >> P
    k = np.asarray(ks, np.int64)[idx // lp]
    first = (idx == o) | (idx % lp == 0)
    q = u >> k
    length = q + 1 + k + 4 * first
    start = 8 + 16 * o + 6 + np.concatenate([[0], np.cumsum(length)[:-1]])
    total = 8 + 16 * o + 6 + int(length.sum())
    pos = [np.array([0]), 8 + 16 * np.arange(o), np.array([8 + 16 * o]), start[first], start + 4 * first + q]
    lens = [np.array([8]), np.full(o, 16), np.array([6]), np.full(int(first.sum()), 4), k + 1]
    vals = [np.array([(8 | o) << 1]), x[:o] & 0xFFFF, np.array([P]), k[first], (1 << k) | (u & ((1 << k) - 1))]
    return pack_fields(np.concatenate(pos), np.concatenate(lens), np.concatenate(vals), total), total


def seek_frames(n, seek_interval):
    """The frames a seek table names: t = 0, interval, .. < n -> t // 4096, a repeat of the previous point's frame skipped."""
    if seek_interval <= 0:
        return []
    if seek_interval >= BLOCK:
        return [t // BLOCK for t in range(0, n, seek_interval)]
    return list(range(((n - 1) // seek_interval * seek_interval) // BLOCK + 1))      # every frame up to the last multiple's, once


def encode(x, rate, seek_interval=0, info=False):
    x = np.asarray(x)
    assert x.dtype == np.int16 and x.ndim == 1 and x.size >= 1
    n = x.size
    x = x.astype(np.int64)
    F = (n + BLOCK - 1) // BLOCK
    blocks = [x[f * BLOCK:(f + 1) * BLOCK] for f in range(F)]
    const = [bool((b == b[0]).all()) for b in blocks]
    records = [None] * F
    for bs in sorted({b.size for b in blocks}):
        sel = [f for f in range(F) if blocks[f].size == bs and not const[f]]
        if sel:
            bits, o, P, ks = analyse(np.stack([blocks[f] for f in sel]))
            for j, f in enumerate(sel):
                records[f] = (int(bits[j]), int(o[j]), int(P[j]), ks[j, :1 << int(P[j])].tolist())
    frames, infos = [], []
    for f, b in enumerate(blocks):
        if const[f]:
            kind, (body, bits), o, P, ks = "CONSTANT", subframe(b, "CONSTANT"), 0, 0, []
        else:
            fbits, o, P, ks = records[f]
            if fbits < 8 + 16 * b.size:
                kind, (body, bits) = "FIXED", subframe(b, "FIXED", o, P, ks)
                assert bits == fbits
            else:
                kind, (body, bits), o, P, ks = "VERBATIM", subframe(b, "VERBATIM"), 0, 0, []
        head = frame_header(f, b.size, rate)
        fr = head + body
        fr += crc16(fr).to_bytes(2, "big")
        frames.append(fr)
        infos.append(dict(kind=kind, order=o, porder=P, ks=ks, bs=b.size, bits=bits, bytes=len(fr), number_bytes=len(coded_number(f)),
                          bs_code=head[2] >> 4, rate_code=head[2] & 15))
    sizes = [len(fr) for fr in frames]
    rel = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    pts = seek_frames(n, seek_interval)
    si = (BLOCK.to_bytes(2, "big") * 2 + min(sizes).to_bytes(3, "big") + max(sizes).to_bytes(3, "big")
          + ((rate << 44) | (0 << 41) | (15 << 36) | n).to_bytes(8, "big") + bytes(16))
    out = b"fLaC" + bytes([0x00 if pts else 0x80]) + (34).to_bytes(3, "big") + si
    if pts:
        out += bytes([0x83]) + (18 * len(pts)).to_bytes(3, "big")
        for f in pts:
            out += (f * BLOCK).to_bytes(8, "big") + rel[f].to_bytes(8, "big") + blocks[f].size.to_bytes(2, "big")
    out += b"".join(frames)
    return (out, infos) if info else out


def encode_batch(clips, rate, factor=None, seek_interval=0):
    streams = [encode(c if factor is None else loudref.apply_gain(c, float(factor[i])), rate, seek_interval) for i, c in enumerate(clips)]
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.uint64)
    return b"".join(streams), offsets
