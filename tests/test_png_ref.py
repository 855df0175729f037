"""The PNG encoder's restatement (tests/pngref.py, written from DESIGN.md §9 "PNG") against an independent reader (tests/pngdec.py,
whose inflater is zlib's), and the C ABI's argument checks, which need no device."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import birdnet_go_amd  # noqa: F401
from birdnet_go_amd import host

import pngcases as K
import pngdec
import pngref

ENTRIES = ("bnhip_png_max_bytes", "bnhip_png_workspace_size", "bnhip_png_encode_device", "bnhip_png_encode_u8", "bnhip_spectrogram_png_pcm16")


def streams(name):
    data, off = K.reference(name)
    return [data[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]


@pytest.mark.parametrize("name", K.NAMES)
def test_restated_stream_decodes_to_its_image_and_palette(name):
    images, forms = K.cases()[name]
    ss = streams(name)
    assert len(ss) == len(images)
    for im, s in zip(images, ss):
        idx, pal = pngdec.decode(s)
        assert np.array_equal(idx, im) and np.array_equal(pal, K.palette()), name
        assert len(s) <= pngref.max_bytes(1, im.shape[1], im.shape[0])
    assert sum(map(len, ss)) <= pngref.max_bytes(len(images), images.shape[2], images.shape[1])
    if forms is not None:
        got = []
        pngref.encode(images[0], K.palette(), got)
        assert got == forms, (name, [pngref.FORM_NAMES[f] for f in got])
        assert pngref.band_count(images.shape[2], images.shape[1]) == len(forms)


def test_the_mixed_batch_takes_every_form():
    images, _ = K.cases()["batch300"]
    seen = []
    for im in images[:3]:
        pngref.encode(im, K.palette(), seen)
    assert seen == [pngref.ZERO, pngref.HUFFMAN, pngref.STORED]
    got = []
    pngref.encode(K.cases()["three_images"][0][2], K.palette(), got)
    assert got == [pngref.STORED]


def test_band_rule():
    assert pngref.band_rows(1026, 513) == 16 and pngref.band_count(1026, 513) == 33
    assert pngref.band_rows(4096, 4096) == 4 and pngref.band_rows(1, 4096) == 4096 and pngref.band_rows(7, 4096) == 2048
    assert pngref.band_rows(16383, 5) == 1 and pngref.band_rows(300, 1) == 1
    worst = max(pngref.band_rows(w, 4096) * (w + 1) for w in range(1, 4097))
    assert worst <= 20481


def test_stored_is_the_bound_of_every_form():
    """A ZERO band is shorter than STORED whenever it can occur: a band that is not the last holds at least 16384 bytes."""
    for n in list(range(2, 600)) + [16384, 20481]:
        for final in (True, False):
            if not final and n < 16384:
                continue
            form, data = pngref.encode_band(np.zeros(n, np.uint8), final)
            assert form == pngref.ZERO and len(data) < 5 + n
            assert zlib.decompressobj(-15).decompress(data + (b"" if final else b"\x01\x00\x00\xff\xff")) == bytes(n)


def kraft(lens):
    return sum(2.0 ** -l for l in lens if l)


def test_fibonacci_counts_drive_the_15_bit_limit():
    image = K.cases()["fibonacci"][0][0]
    rows = np.zeros((192, 57), np.uint8)
    rows[:, 1:] = image
    counts = np.bincount(rows.reshape(-1), minlength=256).tolist() + [1]
    assert sum(1 for c in counts[:256] if c) >= 18
    _, depths = pngref.huffman_depths(counts)
    assert max(depths) == 18                                     # plain Huffman would not fit a DEFLATE code
    lens = pngref.code_lengths(counts, 15)
    assert max(lens) == 15 and kraft(lens) == 1.0
    assert [l > 0 for l in lens] == [c > 0 for c in counts]
    # the rarer symbol never has the shorter code
    order = sorted((s for s in range(257) if counts[s]), key=lambda s: (counts[s], s))
    assert all(lens[a] >= lens[b] for a, b in zip(order, order[1:]))


def test_code_length_code_limit_of_7_on_a_contrived_histogram():
    """Lengths 0..15 with Fibonacci counts (sum 2583 - far more than a real header's 258 lengths, which is why this is driven here
    and not on the device): plain Huffman reaches depth 15, the rule returns a complete code of at most 7 bits."""
    counts = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 0, 0, 0]
    _, depths = pngref.huffman_depths(counts)
    assert max(depths) == 15
    lens = pngref.code_lengths(counts, 7)
    assert max(lens) == 7 and kraft(lens) == 1.0 and lens[16:] == [0, 0, 0]
    assert all(lens[i] >= lens[i + 1] for i in range(15))
    # a histogram a header can have (258 lengths) that still needs the limit: 1, 1, 2, 3, 5, 8, 13, 21, 34, 170
    counts = [1, 1, 2, 3, 5, 8, 13, 21, 34, 170] + [0] * 9
    assert sum(counts) == 258 and max(pngref.huffman_depths(counts)[1]) == 9
    lens = pngref.code_lengths(counts, 7)
    assert max(lens) == 7 and kraft(lens) == 1.0
    # no limit in the way: plain Huffman's cost
    counts = [5, 9, 12, 13, 16, 45]
    assert sum(c * l for c, l in zip(counts, pngref.code_lengths(counts, 15))) == 224
    assert pngref.code_lengths([0, 7, 0, 3], 15) == [0, 1, 0, 1]


def test_canonical_codes_of_the_rfc_example():
    assert pngref.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4]) == [2, 3, 4, 5, 6, 0, 14, 15]


def test_the_reader_rejects_corruptions():
    s = bytearray(streams("two_values")[0])
    assert pngdec.decode(bytes(s))[0].shape == (40, 50)
    for pos in (3, 20, 40, 900, len(s) - 30, len(s) - 14, len(s) - 2):
        bad = bytearray(s)
        bad[pos] ^= 0x10
        with pytest.raises(pngdec.PngError):
            pngdec.decode(bytes(bad))
    with pytest.raises(pngdec.PngError):
        pngdec.decode(bytes(s) + b"\x00")
    # a wrong Adler-32 behind correct CRCs
    kinds = pngdec.chunks(bytes(s))
    body = bytearray(kinds[2][1])
    body[-1] ^= 1
    forged = pngref.SIGNATURE + b"".join(pngref.chunk(k, bytes(body) if k == b"IDAT" else b) for k, b in kinds)
    with pytest.raises(pngdec.PngError, match="inflate"):
        pngdec.decode(forged)


def test_the_reader_undoes_the_other_filters():
    """zlib's own stream with rows of filter types 1..4 (the encoder never writes them)."""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (5, 9)).astype(np.int64)
    rows = bytearray()
    for y in range(5):
        f = y % 5
        up = img[y - 1] if y else np.zeros(9, np.int64)
        rows.append(f)
        for x in range(9):
            a = img[y, x - 1] if x else 0
            c = up[x - 1] if x else 0
            pred = (0, a, up[x], (a + up[x]) // 2, pngdec._paeth(a, up[x], c))[f]
            rows.append(int(img[y, x] - pred) & 255)
    s = (pngref.SIGNATURE + pngref.chunk(b"IHDR", b"\x00\x00\x00\x09\x00\x00\x00\x05\x08\x03\x00\x00\x00")
         + pngref.chunk(b"PLTE", K.palette().tobytes()) + pngref.chunk(b"IDAT", zlib.compress(bytes(rows))) + pngref.chunk(b"IEND", b""))
    assert np.array_equal(pngdec.decode(s)[0], img)


# ---------------------------------------------------------------------------------------------------- C ABI, no device needed
def test_png_symbols_are_exported(built_lib):
    lib = host.load_library()
    for s in ENTRIES:
        assert s in host.SYMBOLS and getattr(lib, s)


def test_go_shim_declares_and_binds_the_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shim_dir = os.path.join(root, "birdnet-go_amd", "go", "internal", "inference", "hip")
    shim = open(os.path.join(shim_dir, "backend_hip.go")).read()
    stub = open(os.path.join(shim_dir, "stub_nohip.go")).read()
    for s in ("bnhip_png_max_bytes", "bnhip_png_encode_u8", "bnhip_spectrogram_png_pcm16"):
        assert f'"{s}"' in shim, s
    for fn in ("func EncodePNG(", "func RenderSpectrogramPNGs("):
        b = shim[shim.index(fn):]
        b = b[:b.index("\n}\n")]
        assert "runtime.LockOSThread()" in b and "defer runtime.UnlockOSThread()" in b and "lastError()" in b, fn
        assert fn in stub


def test_max_bytes_and_workspace_size_answers(built_lib):
    for n, w, h in ((1, 1, 1), (3, 7, 4096), (64, 1026, 513), (2, 4096, 4096), (65535, 5, 3)):
        assert host.png_max_bytes(n, w, h) == pngref.max_bytes(n, w, h)
        assert host.png_workspace_size(n, w, h) > 0
    lib = host.load_library()
    need = C.c_size_t(0)
    for fn in (lib.bnhip_png_max_bytes, lib.bnhip_png_workspace_size):
        assert fn(C.c_int(1), C.c_int(8), C.c_int(8), None) == host.E_INVALID
        for bad in ((0, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 4097, 8), (1, 8, 0), (1, 8, 4097)):
            assert fn(*map(C.c_int, bad), C.byref(need)) == host.E_INVALID, bad


def test_png_argument_errors_before_any_device(built_lib):
    lib = host.load_library()
    ci, cd, vp, sz = C.c_int, C.c_double, C.c_void_p, C.c_size_t
    img = np.zeros(64 * 64, np.uint8)
    pal = np.zeros(768, np.uint8)
    outb = np.zeros(1 << 16, np.uint8)
    offs = np.zeros(8, np.uint64)
    pcm = np.zeros(4096, np.int16)
    i, p, o, f, x = (vp(a.ctypes.data) for a in (img, pal, outb, offs, pcm))
    dev = ci(99)                                                             # no such device: a valid call would fail differently
    cap, ws = host.png_max_bytes(1, 20, 33), host.png_workspace_size(1, 20, 33)

    def u8(images=i, n=1, w=20, h=33, palette=p, out=o, out_cap=cap, offsets=f):
        return lib.bnhip_png_encode_u8(dev, images, ci(n), ci(w), ci(h), palette, out, sz(out_cap), offsets)

    def device(images=i, n=1, w=20, h=33, palette=p, out=o, out_cap=cap, offsets=f, wsp=i, ws_bytes=ws):
        return lib.bnhip_png_encode_device(dev, images, ci(n), ci(w), ci(h), palette, out, sz(out_cap), offsets, wsp, sz(ws_bytes), vp())

    def fused(images=x, n=1, w=20, h=33, palette=p, out=o, out_cap=cap, offsets=f, samples=3000, top=0.0, rng=100.0):
        return lib.bnhip_spectrogram_png_pcm16(dev, images, ci(n), ci(samples), ci(24000), ci(0), ci(w), ci(h), vp(), cd(top), cd(rng), palette,
                                               out, sz(out_cap), offsets)

    for fn in (u8, device, fused):
        assert fn(images=vp()) == host.E_INVALID and lib.bnhip_last_error() == b"NULL/empty argument"
        assert fn(palette=vp()) == host.E_INVALID and fn(out=vp()) == host.E_INVALID and fn(offsets=vp()) == host.E_INVALID
        for bad in (0, -1, 65536):
            assert fn(n=bad) == host.E_INVALID
        assert fn(w=0) == host.E_INVALID and fn(w=4097) == host.E_INVALID and b"width" in lib.bnhip_last_error()
        assert fn(h=0) == host.E_INVALID and fn(h=4097) == host.E_INVALID and b"height" in lib.bnhip_last_error()
        assert fn(out_cap=cap - 1) == host.E_INVALID and b"out_cap" in lib.bnhip_last_error()
        assert fn() != host.BNHIP_OK and b"out_cap" not in lib.bnhip_last_error()      # valid arguments reach the device check
    assert device(wsp=vp()) == host.E_INVALID
    assert device(ws_bytes=ws - 1) == host.E_INVALID and b"workspace" in lib.bnhip_last_error()
    odd = img.ctypes.data + 2 if (img.ctypes.data + 2) % 256 else img.ctypes.data + 4
    assert device(wsp=vp(odd)) == host.E_INVALID and b"aligned" in lib.bnhip_last_error()
    # the spectrogram's own limits hold in the fused entry alone
    assert fused(h=34) == host.E_INVALID and b"2^k + 1" in lib.bnhip_last_error()
    assert fused(samples=0) == host.E_INVALID and fused(rng=0.0) == host.E_INVALID
    assert u8(h=34, out_cap=host.png_max_bytes(1, 20, 34)) != host.BNHIP_OK and b"height" not in lib.bnhip_last_error()
