"""Spectrogram images of ragged bursts on the device (bnhip_spectrogram_ragged_pcm16 / _device, bnhip_spectrogram_png_ragged_pcm16):
every clip against the float64 restatement tests/specref.py under test_spectrogram.py's acceptance rule, and byte for byte against
the uniform entry on that clip alone.  The bursts are tests/specraggedcases.py's: each is rendered once, shared and never written."""
import ctypes as C
import functools
import hashlib

import numpy as np
import pytest

import specraggedcases as K
import specref
from birdnet_go_amd import host, spectrogram as sg

from test_parity_gpu import _DevBuf
from test_spectrogram import A, render, shape_a
from test_spectrogram_ref import decode_png

pytestmark = pytest.mark.gpu
RATE = K.RATE


def _lib():
    lib = host.load_library()
    lib.bnhip_spectrogram_ragged_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                   C.c_double, C.c_double, C.c_void_p]
    lib.bnhip_spectrogram_png_ragged_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                       C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return lib


def render_ragged(clips, width, height, rate_in=RATE, rate_out=0):
    """The host entry with an explicit height (host.spectrogram_ragged derives it from the width)."""
    lib = _lib()
    x, lens = host.ragged_pack(clips)
    img = np.full((lens.size, height, width), 0xAA, np.uint8)
    rc = lib.bnhip_spectrogram_ragged_pcm16(0, x.ctypes.data, lens.size, lens.ctypes.data, rate_in, rate_out, width, height, None, 0.0, 100.0,
                                            img.ctypes.data)
    assert rc == host.BNHIP_OK, lib.bnhip_last_error()
    img.setflags(write=False)
    return img


def render_png_ragged(clips, width, height, palette, rate_in=RATE, rate_out=0, cap=None):
    """-> (rc, streams back to back, offsets) of the fused entry with an explicit height"""
    lib = _lib()
    x, lens = host.ragged_pack(clips)
    pal = np.ascontiguousarray(palette, np.uint8).reshape(-1)
    full = host.png_max_bytes(lens.size, width, height)
    out, offsets = np.zeros(full, np.uint8), np.zeros(lens.size + 1, np.uint64)
    rc = lib.bnhip_spectrogram_png_ragged_pcm16(0, x.ctypes.data, lens.size, lens.ctypes.data, rate_in, rate_out, width, height, None, 0.0,
                                                100.0, pal.ctypes.data, out.ctypes.data, full if cap is None else cap, offsets.ctypes.data)
    return rc, out, offsets


@functools.lru_cache(maxsize=None)
def ragged_image(name):
    width, height, clips = K.burst(name)
    return render_ragged(clips, width, height)


@functools.lru_cache(maxsize=None)
def resampled_image():
    R = K.RESAMPLED
    return render_ragged(K.resampled_burst(), R["width"], R["height"], R["rate_in"], R["rate_out"])


@pytest.mark.parametrize("name", K.COMPARED)
def test_every_clip_meets_the_restatement(gpu, name):
    width, height, clips = K.burst(name)
    img = ragged_image(name)
    shares = [specref.compare(img[i], np.asarray(c, np.float64) / 32768.0, width, height) for i, c in enumerate(clips)]
    print(f"{name}: W={width} H={height} clips={len(clips)}: excused share max {max(shares):.3g}")


@pytest.mark.parametrize("name", list(K.BURSTS))
def test_every_clip_equals_the_uniform_entry_on_that_clip_alone(gpu, name):
    width, height, clips = K.burst(name)
    img = ragged_image(name)
    assert img.shape == (len(clips), height, width)
    for i, c in enumerate(clips):
        assert np.array_equal(img[i], render(c, width, height)[0]), (name, i, c.size)


def test_one_length_equals_the_uniform_batch(gpu):
    clips, img = shape_a()
    assert np.array_equal(render_ragged(list(clips[:5]), A["width"], A["height"]), img[:5])
    assert np.array_equal(host.spectrogram_ragged(list(clips[:5]), RATE, A["width"]), img[:5])


def device_render_ragged(data, f32, lens, width, height):
    ws = host.spectrogram_ragged_workspace_size(lens, width)
    d_in, d_img, d_ws = _DevBuf(data.nbytes), _DevBuf(len(lens) * height * width), _DevBuf(ws)
    try:
        d_in.upload(data)
        host.spectrogram_ragged_device(d_in.ptr, f32, lens, width, height, d_img.ptr, d_ws.ptr, ws)
        return d_img.download((len(lens), height, width), np.uint8)
    finally:
        d_in.free(); d_img.free(); d_ws.free()


def test_device_entry_equals_the_host_entry(gpu):
    width, height, clips = K.burst("a")                          # (258 -> 129: the wrapper's height)
    packed, lens = host.ragged_pack(clips)
    assert np.array_equal(device_render_ragged(packed, False, lens, width, height), ragged_image("a"))
    # packed float32 at the render rate, from the resampler the host entry runs on the device
    R = K.RESAMPLED
    rs = host.Resampler(R["rate_in"], R["rate_out"])
    parts = [rs.resample_f32(c.astype(np.float32)[None, :] / np.float32(32768.0))[0] for c in K.resampled_burst()]
    assert all(p.dtype == np.float32 for p in parts) and len({p.size for p in parts}) == len(parts)
    got = device_render_ragged(np.concatenate(parts), True, [p.size for p in parts], R["width"], R["height"])
    assert np.array_equal(got, resampled_image())
    for i, p in enumerate(parts):
        specref.compare(got[i], p.astype(np.float64), R["width"], R["height"])


def test_device_entry_refuses_a_short_or_misaligned_workspace(gpu):
    width, height, clips = K.burst("odd")
    packed, lens = host.ragged_pack(clips)
    need = K.workspace_bytes(len(clips))
    lib = host.load_library()
    lib.bnhip_spectrogram_ragged_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double,
                                                    C.c_double, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    d_in, d_img, d_ws = _DevBuf(packed.nbytes), _DevBuf(len(clips) * height * width), _DevBuf(need + 256)
    try:
        d_in.upload(packed)
        go = lambda ws_ptr, ws: lib.bnhip_spectrogram_ragged_device(0, d_in.ptr, 0, lens.size, lens.ctypes.data, width, height, None, 0.0, 100.0,
                                                                    d_img.ptr, ws_ptr, ws, None)
        assert go(d_ws.ptr, need - 1) == host.E_INVALID and b"workspace" in lib.bnhip_last_error()
        assert go(d_ws.at(128), need) == host.E_INVALID and b"aligned" in lib.bnhip_last_error()
        assert go(d_ws.ptr, need) == host.BNHIP_OK
        assert np.array_equal(d_img.download((len(clips), height, width), np.uint8), ragged_image("odd"))
    finally:
        d_in.free(); d_img.free(); d_ws.free()


def test_resampled_every_clip_equals_the_uniform_entry(gpu):
    R, clips, img = K.RESAMPLED, K.resampled_burst(), resampled_image()
    for i, c in enumerate(clips):
        alone = render(c, R["width"], R["height"], rate_in=R["rate_in"], rate_out=R["rate_out"])
        assert np.array_equal(img[i], alone[0]), (i, c.size)
    # rate_out == rate_in renders at the source rate, like rate_out == 0
    same = render_ragged(clips, R["width"], R["height"], R["rate_in"], R["rate_in"])
    assert np.array_equal(same, render_ragged(clips, R["width"], R["height"], R["rate_in"], 0))
    assert not np.array_equal(same, img)


@pytest.mark.parametrize("which", ["a", "resampled"])
def test_fused_png_entry(gpu, which, tmp_path):
    if which == "a":
        width, height, clips = K.burst("a")
        rates, img = dict(rate_in=RATE, rate_out=0), ragged_image("a")
    else:
        R = K.RESAMPLED
        width, height, clips = R["width"], R["height"], K.resampled_burst()
        rates, img = dict(rate_in=R["rate_in"], rate_out=R["rate_out"]), resampled_image()
    pal = sg.palette("default")
    rc, out, offsets = render_png_ragged(clips, width, height, pal, **rates)
    assert rc == host.BNHIP_OK
    want, want_off = host.png_encode(img, pal, raw=True)                     # bnhip_png_encode_u8 of the ragged render's images
    assert np.array_equal(offsets, want_off) and offsets[0] == 0 and int(offsets[-1]) == want.size
    assert np.array_equal(out[:want.size], want)
    assert (np.diff(offsets.astype(np.int64)) > 0).all()
    for i in range(len(clips)):
        p = tmp_path / f"{i}.png"
        p.write_bytes(out[int(offsets[i]):int(offsets[i + 1])].tobytes())
        idx, gpal = decode_png(p)
        assert np.array_equal(idx, img[i]) and np.array_equal(gpal, pal)
    if which == "a":
        streams = host.spectrogram_png_ragged(clips, RATE, width, pal)       # the wrapper: the same streams as a list
        assert [len(s) for s in streams] == np.diff(offsets.astype(np.int64)).tolist()
        assert b"".join(streams) == want.tobytes()


def test_fused_png_entry_refuses_a_short_out_cap(gpu):
    width, height, clips = K.burst("odd")
    cap = host.png_max_bytes(len(clips), width, height)
    rc, _, _ = render_png_ragged(clips, width, height, sg.palette("default"), cap=cap - 1)
    assert rc == host.E_INVALID and b"out_cap" in host.load_library().bnhip_last_error()
    assert render_png_ragged(clips, width, height, sg.palette("default"), cap=cap)[0] == host.BNHIP_OK


def _read_back(paths):
    return np.stack([decode_png(p)[0] for p in paths])


def test_generate_burst_every_way_writes_the_same_indices(gpu, tmp_path):
    lens = (72000, 5001, 72000, 257, 66049, 5001)
    clips = [K.signal(K.SIGNALS[i % 6], n, seed=i // 6) for i, n in enumerate(lens)]
    prof = sg.FrequencyProfile(0)
    want = host.spectrogram_ragged(clips, RATE, 258)
    for i, c in enumerate(clips):
        assert np.array_equal(want[i], host.spectrogram(c, RATE, 258)[0])
    for ragged in (False, True):
        for device_png in (False, True):
            paths = [str(tmp_path / f"r{int(ragged)}p{int(device_png)}_{i}.png") for i in range(len(clips))]
            got = sg.generate_burst(clips, paths, 258, RATE, profile=prof, device_png=device_png, ragged=ragged)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (ragged, device_png)
            assert np.array_equal(_read_back(paths), want), (ragged, device_png)
    # through the bird profile's resampler, with a style that brings its own window and range
    paths = [str(tmp_path / f"bird{i}.png") for i in range(len(clips))]
    a = sg.generate_burst(clips, paths, 258, 48000, style="scientific", dynamic_range="80", ragged=True, device_png=True)
    b = sg.generate_burst(clips, paths, 258, 48000, style="scientific", dynamic_range="80")
    assert np.array_equal(a, b) and np.array_equal(_read_back(paths), b) and np.array_equal(decode_png(paths[0])[1], sg.palette("scientific"))
    # all lengths equal: generate_batch's result
    same, spaths = shape_a()[0][:3], [str(tmp_path / f"same{i}.png") for i in range(3)]
    batch = sg.generate_batch(same, spaths, 258, RATE, profile=prof)
    for ragged in (False, True):
        assert np.array_equal(sg.generate_burst(list(same), spaths, 258, RATE, profile=prof, ragged=ragged), batch)
        assert np.array_equal(_read_back(spaths), batch)


# sha256 of the uint8 [6, 129, 258] image test_spectrogram.shape_a() renders (bnhip_spectrogram_pcm16, six signals of 72 000 samples at
# 258 x 129), taken on an MI355X from the library built from the parent of the commit that added the ragged entries (build.py with
# BNHIP_LIBDIR on that tree's csrc, loaded with host.load_library(path)); the uniform launch must keep giving these bytes.
SHAPE_A_SHA256_PARENT = "38c5cefc2ee24647e5e3ed0d5fe50ef60cbf1c8f8c072af974fe31f52a934d94"


def test_uniform_entry_is_unchanged(gpu):
    _, img = shape_a()
    assert img.shape == (6, 129, 258)
    assert hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest() == SHAPE_A_SHA256_PARENT
