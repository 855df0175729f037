"""The PNG encoder of DESIGN.md §9 "PNG", restated in Python integers and numpy from that text (not from the kernels): an 8-bit
indexed image, filter 0 on every row, one IDAT chunk per band, each band a byte-aligned piece of one DEFLATE stream in one of three
forms (ZERO, HUFFMAN, STORED).  Every byte is pinned."""
import struct
import zlib

import numpy as np

ZERO, HUFFMAN, STORED = 0, 1, 2
FORM_NAMES = {ZERO: "ZERO", HUFFMAN: "HUFFMAN", STORED: "STORED"}
BAND_TARGET = 16384
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
SIGNATURE = b"\x89PNG\r\n\x1a\n"
ADLER = 65521
# RFC 1951 §3.2.5: the length symbols' base lengths and extra bits, symbols 257..285
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)


def band_rows(width, height):
    return max(1, min(height, -(-BAND_TARGET // (width + 1))))


def band_count(width, height):
    return -(-height // band_rows(width, height))


def max_bytes(n_images, width, height):
    """The bound of every buffer: every band STORED."""
    per = 8 + 25 + 780 + 12 + 2 + 4 + band_count(width, height) * (12 + 5) + height * (width + 1)
    return n_images * per


def huffman_depths(counts):
    """Plain Huffman depths of the symbols with a non-zero count (at least two of them), by the spec's two-queue rule: leaves in
    ascending (count, symbol) order, internal nodes in the order they were made, a leaf before an internal node of equal weight.
    -> (order, depths): the symbols in leaf order and each one's depth."""
    order = sorted((s for s, c in enumerate(counts) if c > 0), key=lambda s: (counts[s], s))
    m = len(order)
    assert m >= 2
    weight = [counts[s] for s in order] + [0] * (m - 1)
    parent = [0] * (2 * m - 1)
    li, ii, nxt = 0, m, m
    for _ in range(m - 1):
        pick = []
        for _ in range(2):
            if li < m and (ii >= nxt or weight[li] <= weight[ii]):
                pick.append(li)
                li += 1
            else:
                pick.append(ii)
                ii += 1
        weight[nxt] = weight[pick[0]] + weight[pick[1]]
        parent[pick[0]] = parent[pick[1]] = nxt
        nxt += 1
    depths = []
    for p in range(m):
        d, node = 0, p
        while node != 2 * m - 2:
            node = parent[node]
            d += 1
        depths.append(d)
    return order, depths


def code_lengths(counts, limit):
    """Code lengths of an alphabet, at most `limit` bits: Huffman depths, folded onto `limit`, the Kraft sum repaired one unit at a
    time, then the lengths handed out again in count order.  -> list of len(counts) lengths, 0 for an absent symbol."""
    order, depths = huffman_depths(counts)
    m = len(order)
    blc = [0] * (limit + 1)
    for d in depths:
        blc[min(d, limit)] += 1
    total = sum(blc[i] << (limit - i) for i in range(1, limit + 1))
    while total != 1 << limit:
        blc[limit] -= 1
        for i in range(limit - 1, 0, -1):
            if blc[i]:
                blc[i] -= 1
                blc[i + 1] += 2
                break
        total -= 1
    lens = [0] * len(counts)
    for p, s in enumerate(order):
        q = m - 1 - p                      # the rank from the most frequent end; of equal counts the larger symbol ranks first
        l, acc = 1, blc[1]
        while acc <= q:
            l += 1
            acc += blc[l]
        lens[s] = l
    return lens


def canonical_codes(lens):
    """RFC 1951 §3.2.2."""
    top = max(lens)
    blc = [0] * (top + 2)
    for l in lens:
        if l:
            blc[l] += 1
    nxt, code = [0] * (top + 2), 0
    for b in range(1, top + 1):
        code = (code + blc[b - 1]) << 1
        nxt[b] = code
    codes = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


def _rev(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


class Bits:
    """LSB-first bit writer."""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, n):                   # a plain field: least significant bit first
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n

    def code(self, c, n):                  # a Huffman code: most significant bit first
        self.put(_rev(c, n), n)

    def align(self):
        self.n = (self.n + 7) & ~7

    def tobytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def dynamic_tables(band):
    """-> (lens[257], cl_lens[19], ncl, bits of the whole dynamic block) of a band's bytes."""
    counts = np.bincount(band, minlength=256).tolist() + [1]
    lens = code_lengths(counts, 15)
    seq = lens + [1]                       # HLIT 0: 257 literal/length lengths; HDIST 0: one distance code, of one bit, never used
    cl_counts = [0] * 19
    for l in seq:
        cl_counts[l] += 1
    cl_lens = code_lengths(cl_counts, 7)
    ncl = max(i for i, s in enumerate(CL_ORDER) if cl_lens[s]) + 1
    bits = 3 + 5 + 5 + 4 + 3 * ncl + sum(cl_lens[l] for l in seq) + sum(c * l for c, l in zip(counts, lens))
    return lens, cl_lens, ncl, bits


def fixed_code(w, sym):
    """A literal/length symbol in the fixed code (RFC 1951 §3.2.6)."""
    if sym < 144:
        w.code(0x30 + sym, 8)
    elif sym < 256:
        w.code(0x190 + sym - 144, 9)
    elif sym < 280:
        w.code(sym - 256, 7)
    else:
        w.code(0xC0 + sym - 280, 8)


def zero_block(n, final):
    w = Bits()
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    fixed_code(w, 0)
    q, r = divmod(n - 1, 258)
    for _ in range(q):
        fixed_code(w, 285)
        w.code(0, 5)                       # distance 1
    if r >= 3:
        k = max(i for i in range(29) if LEN_BASE[i] <= r)
        fixed_code(w, 257 + k)
        w.put(r - LEN_BASE[k], LEN_EXTRA[k])
        w.code(0, 5)
    else:
        for _ in range(r):
            fixed_code(w, 0)
    fixed_code(w, 256)
    return w


def _closed(w, final):
    """The block's bytes, a non-final one followed by an empty stored block."""
    if final:
        return w.tobytes()
    w.put(0, 3)
    w.align()
    return w.tobytes() + b"\x00\x00\xff\xff"


def huffman_block(band, final, tables):
    lens, cl_lens, ncl, _ = tables
    w = Bits()
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(0, 5)
    w.put(0, 5)
    w.put(ncl - 4, 4)
    for s in CL_ORDER[:ncl]:
        w.put(cl_lens[s], 3)
    cl_codes = canonical_codes(cl_lens)
    for l in lens + [1]:
        w.code(cl_codes[l], cl_lens[l])
    codes = canonical_codes(lens)
    # the literals at once: every byte's reversed code at its running bit position
    rc = np.array([_rev(c, l) for c, l in zip(codes, lens)], np.int64)
    ln = np.array(lens, np.int64)
    bl = ln[band]
    pos = np.cumsum(bl) - bl
    bitsarr = np.zeros(int(bl.sum()), np.uint8)
    for k in range(15):
        m = bl > k
        bitsarr[pos[m] + k] = (rc[band[m]] >> k) & 1
    lit = int.from_bytes(np.packbits(bitsarr, bitorder="little").tobytes(), "little")
    w.acc |= lit << w.n
    w.n += bitsarr.size
    w.code(codes[256], lens[256])
    return w


def encode_band(band, final):
    """-> (form, the band's bytes of the DEFLATE stream)."""
    n = band.size
    stored = bytes([1 if final else 0]) + struct.pack("<HH", n, n ^ 0xFFFF) + band.tobytes()
    if not band.any():
        return ZERO, _closed(zero_block(n, final), final)
    tables = dynamic_tables(band)
    hbytes = (tables[3] + 7) // 8 if final else (tables[3] + 3 + 7) // 8 + 4
    if hbytes < len(stored):
        out = _closed(huffman_block(band, final, tables), final)
        assert len(out) == hbytes
        return HUFFMAN, out
    return STORED, stored


def adler_partial(band):
    """(sum of the bytes, sum of (n - i) * byte[i]) mod 65521."""
    b = band.astype(np.int64)
    return int(b.sum() % ADLER), int((b * np.arange(band.size, 0, -1)).sum() % ADLER)


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode(image, palette, forms=None):
    """uint8 [H, W] indices, uint8 [256, 3] (or [768]) palette -> the PNG stream.  forms: a list that receives each band's form."""
    img = np.ascontiguousarray(image, np.uint8)
    pal = np.ascontiguousarray(palette, np.uint8).reshape(768)
    h, w = img.shape
    rows = np.zeros((h, w + 1), np.uint8)
    rows[:, 1:] = img
    R, nb = band_rows(w, h), band_count(w, h)
    out = [SIGNATURE, chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 3, 0, 0, 0)), chunk(b"PLTE", pal.tobytes())]
    s1, s2 = 1, 0
    for b in range(nb):
        band = rows[b * R:(b + 1) * R].reshape(-1)
        form, data = encode_band(band, b == nb - 1)
        if forms is not None:
            forms.append(form)
        a, bb = adler_partial(band)
        s2 = (s2 + band.size * s1 + bb) % ADLER
        s1 = (s1 + a) % ADLER
        if b == 0:
            data = b"\x78\x01" + data
        if b == nb - 1:
            data = data + struct.pack(">I", (s2 << 16) | s1)
        out.append(chunk(b"IDAT", data))
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


def encode_batch(images, palette):
    """-> (the streams back to back, offsets[n + 1])."""
    streams = [encode(im, palette) for im in images]
    return b"".join(streams), np.concatenate(([0], np.cumsum([len(s) for s in streams]))).astype(np.uint64)
