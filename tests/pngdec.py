"""An independent reader of 8-bit indexed PNG streams: walks the chunks and checks every CRC with zlib.crc32, inflates the joined IDAT
data with zlib.decompress (an inflater this project did not write, which also checks the Adler-32), checks IHDR and PLTE, undoes the
row filters and returns (indices uint8 [H, W], palette uint8 [256, 3])."""
import struct
import zlib

import numpy as np


class PngError(ValueError):
    pass


def chunks(data):
    """-> [(type, payload)] of a whole stream, every CRC checked, nothing before the signature or after IEND."""
    data = bytes(data)
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise PngError("bad signature")
    pos, out = 8, []
    while True:
        if pos + 12 > len(data):
            raise PngError("truncated chunk")
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if pos + 12 + n > len(data):
            raise PngError("chunk runs past the stream")
        body = data[pos + 8:pos + 8 + n]
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != (zlib.crc32(kind + body) & 0xFFFFFFFF):
            raise PngError(f"CRC of {kind!r} at {pos}")
        out.append((kind, body))
        pos += 12 + n
        if kind == b"IEND":
            break
    if pos != len(data):
        raise PngError("bytes after IEND")
    return out


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def decode(data):
    ch = chunks(data)
    kinds = [k for k, _ in ch]
    if kinds[0] != b"IHDR" or kinds[-1] != b"IEND" or ch[-1][1] != b"":
        raise PngError("IHDR must come first and an empty IEND last")
    if kinds.count(b"IHDR") != 1 or kinds.count(b"PLTE") != 1 or kinds.count(b"IEND") != 1 or b"IDAT" not in kinds:
        raise PngError("one IHDR, one PLTE, one IEND and some IDAT are needed")
    first, last = kinds.index(b"IDAT"), len(kinds) - 1 - kinds[::-1].index(b"IDAT")
    if any(k != b"IDAT" for k in kinds[first:last + 1]) or kinds.index(b"PLTE") > first:
        raise PngError("IDAT chunks must be consecutive, after PLTE")
    if len(ch[0][1]) != 13:
        raise PngError("IHDR length")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", ch[0][1])
    if (depth, colour, comp, filt, lace) != (8, 3, 0, 0, 0) or w < 1 or h < 1:
        raise PngError("not an 8-bit indexed, non-interlaced image")
    pal = dict(ch)[b"PLTE"]
    if len(pal) != 768:
        raise PngError("PLTE must hold 256 entries")
    try:
        raw = zlib.decompress(b"".join(b for k, b in ch if k == b"IDAT"))
    except zlib.error as e:
        raise PngError(f"inflate: {e}")
    if len(raw) != h * (w + 1):
        raise PngError("the image data has the wrong length")
    rows = np.frombuffer(raw, np.uint8).reshape(h, w + 1)
    out = np.zeros((h, w), np.uint8)
    for y in range(h):
        f, line = int(rows[y, 0]), rows[y, 1:].astype(np.int64)
        up = out[y - 1].astype(np.int64) if y else np.zeros(w, np.int64)
        if f == 0:
            cur = line
        elif f == 2:
            cur = (line + up) & 255
        elif f in (1, 3, 4):
            cur = np.zeros(w, np.int64)
            for x in range(w):
                a = cur[x - 1] if x else 0
                c = up[x - 1] if x else 0
                cur[x] = (line[x] + (a if f == 1 else (a + up[x]) // 2 if f == 3 else _paeth(a, up[x], c))) & 255
        else:
            raise PngError(f"filter type {f}")
        out[y] = cur
    return out, np.frombuffer(pal, np.uint8).reshape(256, 3).copy()
