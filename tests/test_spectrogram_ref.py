"""Spectrogram images, CPU side: the size table, the float64 restatement's known answers, the Dolph window, the PNG writer, the
palettes, and the C ABI's symbols and argument errors (no device needed).  The device images are compared with the same
restatement in test_spectrogram.py."""
import ctypes as C
import os
import re
import struct
import zlib

import numpy as np
import pytest

import specref
from birdnet_go_amd import host, spectrogram as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC_SYMBOLS = ("bnhip_spectrogram_size", "bnhip_spectrogram_pcm16", "bnhip_spectrogram_device")


# ---------------------------------------------------------------------------------------------- size table
def test_size_table_and_fft_friendly_height():
    # utils.go:21-55: width -> (height, DFT size)
    rows = {"sm": (258, 129, 256), "md": (514, 257, 512), "lg": (1026, 513, 1024), "xl": (2050, 1025, 2048)}
    for size, (w, h, n) in rows.items():
        assert sg.size_to_pixels(size) == w and sg.pixels_to_size(w) == size
        assert sg.fft_friendly_height(w) == h == specref.fft_friendly_height(w) and 2 * (h - 1) == n
    with pytest.raises(ValueError):
        sg.size_to_pixels("xxl")
    with pytest.raises(ValueError):
        sg.pixels_to_size(1000)
    assert (sg.bird_profile().resample_rate, sg.bat_profile().resample_rate) == (24000, 256000)      # frequency_profile.go:13-16
    assert np.array_equal(sg.hann(256), specref.hann(256)) and sg.hann(256)[0] == 0.0 and sg.hann(256)[128] == 1.0


# ---------------------------------------------------------------------------------------------- restatement known answers
W, H, N = 258, 129, 256


def test_full_scale_sine_at_an_eighth_of_the_rate_is_index_255():
    n = 72000
    x = np.sin(2.0 * np.pi * np.arange(n) / 8.0)                 # amplitude 1.0 = full scale, exactly on bin N / 8
    img = specref.render(x, W, H)
    m = specref.frame_centres(n, W, N)                           # [W, K], K = 2 here
    interior = np.flatnonzero(((m - N // 2 >= 0) & (m + N // 2 <= n)).all(axis=1))
    assert len(interior) >= W - 2
    row = H - 1 - N // 8
    assert (img[row, interior] == 255).all()
    assert (img[0, interior] == 0).all() and (img[H - 1, interior] == 0).all()


def test_silence_is_an_all_zero_image():
    assert not specref.render_pcm16(np.zeros(5000, np.int16), 40, H).any()


def test_an_impulse_lights_only_the_columns_whose_frames_contain_it():
    n, pos = 72000, 30011
    pcm = np.zeros(n, np.int16)
    pcm[pos] = 32767
    img = specref.render_pcm16(pcm, W, H)
    m = specref.frame_centres(n, W, N)
    w = specref.hann(N)
    lit = np.array([any(0 <= pos - (mc - N // 2) < N and w[pos - (mc - N // 2)] > 1e-6 for mc in col) for col in m])
    assert 1 <= lit.sum() <= 3
    assert img[:, lit].any(axis=0).all() and not img[:, ~lit].any()
    # a column's spectrum of one impulse is flat
    assert (img[:, lit] == img[0, lit][None, :]).all()


def test_the_mean_of_k_frames_is_the_hand_written_mean():
    n = 200000
    rng = np.random.default_rng(5)
    x = rng.uniform(-1.0, 1.0, n)
    K = specref.frames_per_column(n, W, N)
    assert K == 4
    w = specref.hann(N)
    P = specref.column_power(x, W, H)
    for c in (0, 1, 100, W - 1):
        acc = np.zeros(H)
        for k in range(K):
            m = ((2 * (c * K + k) + 1) * n) // (2 * K * W)
            fr = np.array([x[i] if 0 <= i < n else 0.0 for i in range(m - N // 2, m + N // 2)]) * w
            X = np.fft.rfft(fr)
            acc = acc + (X.real ** 2 + X.imag ** 2) * (2.0 / w.sum()) ** 2
        assert np.array_equal(P[c], acc / K)


def test_fft_and_direct_dft_restatements_agree():
    rng = np.random.default_rng(6)
    x = rng.uniform(-1.0, 1.0, 5001)
    a, va = specref.render(x, 33, H, with_v=True)
    b = specref.render(x, 33, H, direct=True)
    assert ((a == b) | specref.excused(va)).all() and np.abs(a.astype(int) - b.astype(int)).max() <= 1


def test_level_rule():
    v = np.array([-np.inf, -3.0, 0.0, 0.49, 0.5, 254.49, 254.5, 255.0, 300.0])
    assert specref.levels(v).tolist() == [0, 0, 0, 0, 1, 254, 255, 255, 255]
    assert specref.level_value(np.array([1.0, 1e-10, 0.0])).tolist() == [255.0, 0.0, -np.inf]
    assert specref.level_value(np.array([1e-4]), range_db=80.0)[0] == 127.5


# ---------------------------------------------------------------------------------------------- Dolph window
@pytest.mark.parametrize("n", [256, 1024, 255])
def test_dolph_window(n):
    w = sg.dolph(n, 100.0)
    assert w.shape == (n,) and np.allclose(w, w[::-1], rtol=0, atol=1e-12) and w.max() == 1.0 and (w > 0).all()
    S = np.abs(np.fft.rfft(w, 16 * n))
    db = 20.0 * np.log10(np.maximum(S / S[0], 1e-300))
    first_null = np.argmax(np.diff(db) > 0)                      # the main lobe falls monotonically to its first minimum
    assert db[first_null:].max() <= -100.0 + 0.1
    assert db[first_null:].max() >= -100.0 - 0.1                 # equiripple: the side lobes sit AT the design level


# ---------------------------------------------------------------------------------------------- PNG writer and palettes
def png_chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    out, o = [], 8
    while o < len(data):
        n, kind = struct.unpack(">I4s", data[o:o + 8])
        body = data[o + 8:o + 8 + n]
        assert struct.unpack(">I", data[o + 8 + n:o + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        out.append((kind, body))
        o += 12 + n
    return out


def decode_png(path):
    """-> (indices [H, W], palette [256, 3]) of an 8-bit indexed PNG whose scanlines all use filter type 0."""
    ch = png_chunks(open(path, "rb").read())
    assert [k for k, _ in ch][0] == b"IHDR" and ch[-1] == (b"IEND", b"")
    w, h, depth, ctype, comp, flt, lace = struct.unpack(">IIBBBBB", dict(ch)[b"IHDR"])
    assert (depth, ctype, comp, flt, lace) == (8, 3, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b"".join(b for k, b in ch if k == b"IDAT")), np.uint8).reshape(h, w + 1)
    assert not raw[:, 0].any()
    return raw[:, 1:], np.frombuffer(dict(ch)[b"PLTE"], np.uint8).reshape(-1, 3)


@pytest.mark.parametrize("shape", [(129, 258), (7, 33), (1, 1)])
def test_write_png_round_trip(tmp_path, shape):
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, shape).astype(np.uint8)
    pal = sg.palette("default")
    p = tmp_path / "a.png"
    sg.write_png(str(p), img, pal)
    got, gpal = decode_png(p)
    assert got.shape == shape and np.array_equal(got, img) and np.array_equal(gpal, pal)
    with pytest.raises(ValueError):
        sg.write_png(str(p), img, pal[:100])


def test_palettes():
    ends = {"default": ((0, 0, 0), (255, 255, 255)), "high_contrast_dark": ((0, 0, 0), (255, 255, 255)),
            "scientific_dark": ((0, 0, 0), (255, 255, 255)), "scientific": ((255, 255, 255), (0, 0, 0))}
    assert set(ends) == set(sg.STYLES)                           # conf/config.go:252-255
    for style, (bg, full) in ends.items():
        p = sg.palette(style)
        assert p.shape == (256, 3) and p.dtype == np.uint8
        assert tuple(p[0]) == bg and tuple(p[255]) == full, style
        assert len({tuple(r) for r in p}) == 256, style          # every level has its own colour
    grey = sg.palette("scientific_dark")
    assert (grey[:, 0] == np.arange(256)).all() and (grey[:, 0] == grey[:, 1]).all() and (grey[:, 1] == grey[:, 2]).all()
    assert np.array_equal(sg.palette("scientific"), grey[::-1])
    with pytest.raises(ValueError):
        sg.palette("sepia")
    assert sg.style_window("default", 256) is None and sg.style_window("high_contrast_dark", 256) is None
    assert np.array_equal(sg.style_window("scientific", 256, 100.0), sg.dolph(256, 120.0))


# ---------------------------------------------------------------------------------------------- C ABI without a device
def test_symbols_are_declared_and_exported(built_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bnhip.h")).read(), flags=re.S)
    lib = C.CDLL(built_lib)
    for s in SPEC_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, src), f"{s} is not declared in include/bnhip.h"
        assert hasattr(lib, s), f"libbnhip.so does not export {s}"
        assert s in host.SYMBOLS


def test_size_entry(built_lib):
    assert host.spectrogram_size(258) == (129, 256) and host.spectrogram_size(2050) == (1025, 2048)
    assert host.spectrogram_size(4096) == (2049, 4096) and host.spectrogram_size(96) == (65, 128)
    lib = host.load_library()
    h, n = C.c_int(0), C.c_int(0)
    for w in (0, -5, 4097):
        assert lib.bnhip_spectrogram_size(w, C.byref(h), C.byref(n)) == host.E_INVALID
        assert lib.bnhip_last_error() == b"width must be in [1, 4096]"
    assert lib.bnhip_spectrogram_size(258, None, C.byref(n)) == host.E_INVALID and lib.bnhip_last_error() == b"NULL/empty argument"
    assert lib.bnhip_spectrogram_size(20, C.byref(h), C.byref(n)) == host.E_UNSUPPORTED        # height 17: N = 32
    assert (h.value, n.value) == (17, 32) and lib.bnhip_last_error() == b"FFT size 2 * (height - 1) must be in [64, 4096]"


def test_argument_errors_need_no_device(built_lib):
    lib = host.load_library()
    host.spectrogram_size(258)                                   # (declares the size entry's argtypes)
    lib.bnhip_spectrogram_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_double, C.c_double, C.c_void_p]
    lib.bnhip_spectrogram_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double,
                                             C.c_double, C.c_void_p, C.c_void_p]
    pcm = np.zeros((2, 1000), np.int16)
    img = np.zeros((2, 129, 258), np.uint8)
    zero_window = np.zeros(256)
    good = dict(pcm=pcm.ctypes.data, n_clips=2, n=1000, rate_in=48000, rate_out=24000, width=258, height=129, window=None, top_db=0.0,
                range_db=100.0, image=img.ctypes.data)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.bnhip_spectrogram_pcm16(99, a["pcm"], a["n_clips"], a["n"], a["rate_in"], a["rate_out"], a["width"], a["height"],
                                         a["window"], a["top_db"], a["range_db"], a["image"])
        return rc, lib.bnhip_last_error()

    INV, UNS = host.E_INVALID, host.E_UNSUPPORTED
    rows = [
        (dict(pcm=None), INV, b"NULL/empty argument"), (dict(image=None), INV, b"NULL/empty argument"),
        (dict(n_clips=0), INV, b"NULL/empty argument"), (dict(n=0), INV, b"n must be at least 1"),
        (dict(width=0), INV, b"width must be in [1, 4096]"), (dict(width=4097), INV, b"width must be in [1, 4096]"),
        (dict(height=128), INV, b"height must be 2^k + 1"), (dict(height=130), INV, b"height must be 2^k + 1"),
        (dict(height=1), INV, b"height must be 2^k + 1"),
        (dict(range_db=0.0), INV, b"range_db must be finite and positive"), (dict(range_db=-80.0), INV, b"range_db must be finite and positive"),
        (dict(range_db=float("nan")), INV, b"range_db must be finite and positive"), (dict(range_db=float("inf")), INV, b"range_db must be finite and positive"),
        (dict(top_db=float("nan")), INV, b"top_db must be finite"),
        (dict(height=17), UNS, b"FFT size 2 * (height - 1) must be in [64, 4096]"),
        (dict(height=4097), UNS, b"FFT size 2 * (height - 1) must be in [64, 4096]"),
        (dict(window=zero_window.ctypes.data), INV, b"window coefficients sum to zero"),
        (dict(rate_in=0), INV, b"sample rates must be positive"), (dict(rate_out=-1), INV, b"sample rates must be positive"),
    ]
    for kw, code, text in rows:
        assert call(**kw) == (code, text), kw
    # a well-formed call gets as far as the device ordinal
    rc, text = call()
    assert rc in (host.E_INVALID, host.E_NO_DEVICE) and text not in {t for _, _, t in rows}
    # the device entry answers the same checks
    rc = lib.bnhip_spectrogram_device(99, None, 0, 2, 1000, 258, 129, None, 0.0, 100.0, img.ctypes.data, None)
    assert (rc, lib.bnhip_last_error()) == (INV, b"NULL/empty argument")
    rc = lib.bnhip_spectrogram_device(99, pcm.ctypes.data, 0, 2, 1000, 258, 100, None, 0.0, 100.0, img.ctypes.data, None)
    assert (rc, lib.bnhip_last_error()) == (INV, b"height must be 2^k + 1")
    rc = lib.bnhip_spectrogram_device(99, pcm.ctypes.data, 0, 2, 1000, 258, 8193, None, 0.0, 100.0, img.ctypes.data, None)
    assert (rc, lib.bnhip_last_error()) == (UNS, b"FFT size 2 * (height - 1) must be in [64, 4096]")


def test_wrappers_validate_before_the_library(built_lib, tmp_path):
    with pytest.raises(ValueError):
        sg.generate_from_pcm(b"\0\0" * 100, "relative.png", 258, 48000)
    with pytest.raises(ValueError):
        sg.generate_from_pcm(b"\0\0" * 100, str(tmp_path / "a.png"), 258, 48000, dynamic_range="90")
    with pytest.raises(ValueError):
        sg.generate_from_pcm(b"\0\0" * 100, str(tmp_path / "a.png"), 258, 48000, style="sepia")
    with pytest.raises(ValueError):
        sg.generate_from_pcm(b"\0" * 3, str(tmp_path / "a.png"), 258, 48000)
    with pytest.raises(host.HipError):
        host.spectrogram(np.zeros((1, 100), np.int16), 24000, 258, window=np.ones(100))
