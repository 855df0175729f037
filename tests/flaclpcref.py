"""The LPC part of the FLAC encoder spec of DESIGN.md §9 restated: integer sums in int64 / Python ints, the Levinson-Durbin recursion
and the quantisation in plain Python floats, one operation per statement in the spec's order.  Headers, CRCs, the FIXED analysis and
the bit packing are flacref's.  The device's bytes must equal these.

  encode(x, rate, seek_interval=0, lpc_order=0)              -> the stream's bytes (lpc_order 0: flacref.encode's)
  encode(x, rate, seek_interval, lpc_order, info=True)       -> (bytes, [one dict per frame: kind, order, porder, ks, bs, bits, bytes and,
                                                                for a frame that is not constant, `lpc`: what lpc_candidates saw])
  encode_batch(clips, rate, factor, seek, lpc_order)         -> (all streams back to back, offsets uint64 [B + 1])
"""
import math

import numpy as np

import flacref
import loudref

BLOCK = flacref.BLOCK
MAX_ORDER = 8
PRECISION = 12
MAX_SHIFT = 15
MAX_FOLD = 2 * 524280            # the largest folded residual of FIXED order 4 on int16 input: the bound of the uint32 partition sums


def window(bs):
    """A Welch window scaled to 2^14, non-zero at both ends: int64 [bs]."""
    i = np.arange(bs, dtype=np.int64)
    return ((4 * (i + 1) * (bs - i)) << 14) // ((bs + 1) ** 2)


def autocorrelation(x, lags):
    """x int64 [bs] -> Python ints R[0..lags]: xw = (x w) >> 6 (|xw| <= 2^23), R[l] = sum xw[i] xw[i - l] (|R| <= 2^58: exact)."""
    bs = x.size
    xw = (x * window(bs)) >> 6
    return [int((xw[l:] * xw[:bs - l]).sum()) if l < bs else 0 for l in range(lags + 1)]


def levinson(R, mmax):
    """-> ({m: [a_1 .. a_m]} for the orders the recursion reached, whether it stopped on err <= 0)."""
    out = {}
    if R[0] == 0:
        return out, False
    r = [float(v) for v in R]
    err = r[0]
    a = []
    for m in range(1, mmax + 1):
        acc = r[m]
        for j in range(1, m):
            p = a[j - 1] * r[m - j]
            acc = acc - p
        k = acc / err
        new = []
        for j in range(1, m):
            p = k * a[m - j - 1]
            new.append(a[j - 1] - p)
        new.append(k)
        a = new
        kk = k * k
        d = 1.0 - kk
        err = err * d
        out[m] = list(a)
        if not err > 0.0:
            return out, True
    return out, False


def quantise(a):
    """-> (q, shift) or None where the order is not offered."""
    cmax = 0.0
    for v in a:
        if not math.isfinite(v):
            return None
        if abs(v) > cmax:
            cmax = abs(v)
    if cmax == 0.0:
        return None
    _, e = math.frexp(cmax)
    shift = PRECISION - 1 - e
    if shift > MAX_SHIFT:
        shift = MAX_SHIFT
    if shift < 0:
        return None
    scale = float(1 << shift)
    q, e = [], 0.0
    for v in a:
        p = v * scale
        e = e + p
        t = float(round(e))                                  # (ties to even)
        t = -2048.0 if t < -2048.0 else 2047.0 if t > 2047.0 else t
        q.append(int(t))
        e = e - t
    return q, shift


def residual(x, q, shift):
    """x int64 [bs] -> int64 [bs], zero over the m warm-up samples."""
    m, bs = len(q), x.size
    s = np.zeros(bs - m, np.int64)
    for j, c in enumerate(q):
        s += c * x[m - 1 - j:bs - 1 - j]
    assert np.abs(s).max(initial=0) <= 1 << 29
    r = np.zeros(bs, np.int64)
    r[m:] = x[m:] - (s >> shift)
    return r


def rice_search(r, o, head):
    """r int64 [bs] (zero over the o warm-up samples) -> {P: (cost, ks)}: per partition the k in 0..14 of fewest bits, ties to the
    lowest; cost = head + 6 + sum over partitions of (4 + its bits)."""
    bs = r.size
    u = np.where(r >= 0, 2 * r, -2 * r - 1)
    u[:o] = 0
    tz = (bs & -bs).bit_length() - 1
    pmax = min(5, tz)
    fine = np.stack([(u >> k).reshape(1 << pmax, -1).sum(1) for k in range(15)], 1)      # [parts, 15]
    out = {}
    for P in range(pmax, -1, -1):
        if P < pmax:
            fine = fine[0::2] + fine[1::2]
        if (bs >> P) <= o:
            continue
        cnt = np.full(1 << P, bs >> P, np.int64)
        cnt[0] -= o
        bits = (1 + np.arange(15))[None, :] * cnt[:, None] + fine
        out[P] = (head + 6 + int((4 + bits.min(1)).sum()), bits.argmin(1).tolist())
    return out


def lpc_candidates(x, lpc_order):
    """x int64 [bs] -> (candidates {(P, m): (cost, ks)}, coefficients {m: (q, shift)}, what happened on the way)."""
    bs = x.size
    mmax = min(lpc_order, bs - 1)
    R = autocorrelation(x, MAX_ORDER)
    orders, stopped = levinson(R, mmax)
    seen = dict(R0=R[0], mmax=mmax, reached=max(orders, default=0), stopped=stopped, offered=[], over=[], shifts={}, not_offered=[])
    cands, coefs = {}, {}
    for m, a in orders.items():
        qs = quantise(a)
        if qs is None:
            seen["not_offered"].append(m)
            continue
        q, shift = qs
        r = residual(x, q, shift)
        u = np.where(r >= 0, 2 * r, -2 * r - 1)
        if int(u.max()) > MAX_FOLD:
            seen["over"].append(m)
            continue
        seen["offered"].append(m)
        seen["shifts"][m] = shift
        coefs[m] = (q, shift)
        for P, c in rice_search(r, m, 8 + 16 * m + 4 + 5 + PRECISION * m).items():
            cands[P, m] = c
    return cands, coefs, seen


def lpc_subframe(x, m, q, shift, P, ks):
    """-> (bytes, bits) of one LPC subframe of the int64 block x."""
    bs = x.size
    u = residual(x, q, shift)
    u = np.where(u >= 0, 2 * u, -2 * u - 1)[m:]
    idx = np.arange(m, bs)
    lp = bs >> P
    k = np.asarray(ks, np.int64)[idx // lp]
    first = (idx == m) | (idx % lp == 0)
    quo = u >> k
    length = quo + 1 + k + 4 * first
    pre = 8 + 16 * m + 4 + 5 + PRECISION * m
    start = pre + 6 + np.concatenate([[0], np.cumsum(length)[:-1]])
    total = pre + 6 + int(length.sum())
    pos = [np.array([0]), 8 + 16 * np.arange(m), np.array([8 + 16 * m, 8 + 16 * m + 4]), 8 + 16 * m + 9 + PRECISION * np.arange(m),
           np.array([pre]), start[first], start + 4 * first + quo]
    lens = [np.array([8]), np.full(m, 16), np.array([4, 5]), np.full(m, PRECISION), np.array([6]), np.full(int(first.sum()), 4), k + 1]
    vals = [np.array([(32 | (m - 1)) << 1]), x[:m] & 0xFFFF, np.array([PRECISION - 1, shift]), np.asarray(q, np.int64) & 0xFFF, np.array([P]),
            k[first], (1 << k) | (u & ((1 << k) - 1))]
    return flacref.pack_fields(np.concatenate(pos), np.concatenate(lens), np.concatenate(vals), total), total


def encode(x, rate, seek_interval=0, lpc_order=0, info=False):
    x = np.asarray(x)
    assert x.dtype == np.int16 and x.ndim == 1 and x.size >= 1 and 0 <= lpc_order <= MAX_ORDER
    n = x.size
    x = x.astype(np.int64)
    F = (n + BLOCK - 1) // BLOCK
    frames, infos = [], []
    for f in range(F):
        b = x[f * BLOCK:(f + 1) * BLOCK]
        seen = None
        if bool((b == b[0]).all()):
            kind, (body, bits), o, P, ks = "CONSTANT", flacref.subframe(b, "CONSTANT"), 0, 0, []
        else:
            # the list: the FIXED candidates by (P, o), the LPC candidates by (P, m); a later one wins by strictly fewer bits only
            fbits, fo, fP, fk = flacref.analyse(b[None, :])
            best = ("FIXED", int(fbits[0]), int(fo[0]), int(fP[0]), fk[0, :1 << int(fP[0])].tolist())
            if lpc_order:
                cands, coefs, seen = lpc_candidates(b, lpc_order)
                for P in range(6):
                    for m in range(1, MAX_ORDER + 1):
                        if (P, m) in cands and cands[P, m][0] < best[1]:
                            best = ("LPC", cands[P, m][0], m, P, cands[P, m][1])
            kind, cbits, o, P, ks = best
            if cbits >= 8 + 16 * b.size:
                kind, (body, bits), o, P, ks = "VERBATIM", flacref.subframe(b, "VERBATIM"), 0, 0, []
            elif kind == "FIXED":
                body, bits = flacref.subframe(b, "FIXED", o, P, ks)
            else:
                body, bits = lpc_subframe(b, o, coefs[o][0], coefs[o][1], P, ks)
            assert kind == "VERBATIM" or bits == cbits
        head = flacref.frame_header(f, b.size, rate)
        fr = head + body
        fr += flacref.crc16(fr).to_bytes(2, "big")
        frames.append(fr)
        infos.append(dict(kind=kind, order=o, porder=P, ks=ks, bs=b.size, bits=bits, bytes=len(fr), lpc=seen))
    sizes = [len(fr) for fr in frames]
    rel = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
    pts = flacref.seek_frames(n, seek_interval)
    si = (BLOCK.to_bytes(2, "big") * 2 + min(sizes).to_bytes(3, "big") + max(sizes).to_bytes(3, "big")
          + ((rate << 44) | (0 << 41) | (15 << 36) | n).to_bytes(8, "big") + bytes(16))
    out = b"fLaC" + bytes([0x00 if pts else 0x80]) + (34).to_bytes(3, "big") + si
    if pts:
        out += bytes([0x83]) + (18 * len(pts)).to_bytes(3, "big")
        for f in pts:
            out += (f * BLOCK).to_bytes(8, "big") + rel[f].to_bytes(8, "big") + min(BLOCK, n - f * BLOCK).to_bytes(2, "big")
    out += b"".join(frames)
    return (out, infos) if info else out


def encode_batch(clips, rate, factor=None, seek_interval=0, lpc_order=0):
    streams = [encode(c if factor is None else loudref.apply_gain(c, float(factor[i])), rate, seek_interval, lpc_order) for i, c in enumerate(clips)]
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.uint64)
    return b"".join(streams), offsets
