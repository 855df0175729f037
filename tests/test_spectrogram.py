"""Spectrogram images on the device (bnhip_spectrogram_pcm16 / bnhip_spectrogram_device) against the float64 restatement of the
rendering spec, tests/specref.py.

Acceptance rule (specref.compare): the level index is equal at every pixel, except that a pixel whose restated v + 0.5 lies within
1e-6 dB of an integer (2.55e-6 * 100 / range_db level units) may differ by 1; the share of pixels excused this way is capped at
1e-4 per case and the cap is asserted on the restatement before the device image is looked at.

Shapes are the smallest at which each mechanism can go wrong: every transform length's pass structure (N = 64 .. 4096), a batch,
a hop below N, K = 2 and K = 4 frames per column, K above the frames a round holds, an odd width with a partial column tile and
an odd clip count, and a clip shorter than one frame."""
import ctypes as C
import functools

import numpy as np
import pytest

import specref
from birdnet_go_amd import host, spectrogram as sg

from test_parity_gpu import _DevBuf
from test_spectrogram_ref import decode_png

pytestmark = pytest.mark.gpu
RATE = 24000
SIGNALS = ("noise_full", "noise_33", "chirp", "tone", "silence", "impulse")


@functools.lru_cache(maxsize=None)
def signal(name, n, seed=0):
    """int16 [n] at 24 kHz, seeded."""
    rng = np.random.default_rng([seed, SIGNALS.index(name), n])
    t = np.arange(n) / RATE
    if name == "noise_full":
        x = rng.integers(-32768, 32768, n)
    elif name == "noise_33":
        x = rng.integers(-33, 34, n)
    elif name == "chirp":                                        # 200 Hz to Nyquist, linear, amplitude 20 000
        T = n / RATE
        x = np.round(20000.0 * np.sin(2.0 * np.pi * (200.0 * t + (RATE / 2 - 200.0) * t * t / (2.0 * T))))
    elif name == "tone":                                         # full scale at fs / 8
        x = np.round(32767.0 * np.sin(2.0 * np.pi * np.arange(n) / 8.0))
    elif name == "silence":
        x = np.zeros(n)
    else:
        x = np.zeros(n)
        x[(n * 5) // 12] = 32767
    x = x.astype(np.int16)
    x.setflags(write=False)
    return x


def _lib():
    lib = host.load_library()
    lib.bnhip_spectrogram_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_double, C.c_double, C.c_void_p]
    return lib


def render(pcm, width, height, rate_in=RATE, rate_out=0, window=None, top_db=0.0, range_db=100.0):
    """The host entry with an explicit height (host.spectrogram derives it from the width)."""
    lib = _lib()
    x = np.ascontiguousarray(pcm, np.int16)
    x = x[None, :] if x.ndim == 1 else x
    w = None if window is None else np.ascontiguousarray(window, np.float64)
    img = np.full((x.shape[0], height, width), 0xAA, np.uint8)
    rc = lib.bnhip_spectrogram_pcm16(0, x.ctypes.data, x.shape[0], x.shape[1], rate_in, rate_out, width, height,
                                     None if w is None else w.ctypes.data, top_db, range_db, img.ctypes.data)
    assert rc == host.BNHIP_OK, lib.bnhip_last_error()
    return img


def check(img, clips, width, height, **kw):
    shares = [specref.compare(img[i], np.asarray(c, np.float64) / 32768.0, width, height, **kw) for i, c in enumerate(clips)]
    print(f"W={width} H={height} n={len(clips[0])} clips={len(clips)} {kw.get('range_db', 100.0)} dB: excused share max {max(shares):.3g}")


A = dict(width=258, height=129, n=72000)                         # N = 256, K = 2


@functools.lru_cache(maxsize=None)
def shape_a():
    """(clips, device image) of the six signals in one call at shape (a); computed once, shared, never written."""
    clips = np.stack([signal(s, A["n"]) for s in SIGNALS])
    img = render(clips, A["width"], A["height"])
    img.setflags(write=False)
    return clips, img


def test_a_every_signal_as_a_batch_of_six(gpu):
    clips, img = shape_a()
    assert specref.frames_per_column(A["n"], A["width"], 256) == 2
    check(img, clips, A["width"], A["height"])
    # known answers on the device image itself
    tone, silence, impulse = (img[SIGNALS.index(s)] for s in ("tone", "silence", "impulse"))
    assert (tone[129 - 1 - 32, 1:-1] == 255).all() and not silence.any()
    assert 1 <= impulse.any(axis=0).sum() <= 3


@pytest.mark.parametrize("width,height,n,n_clips", [
    (514, 257, 36000, 3),        # (b) N = 512, hop 70 < N
    (96, 513, 24000, 3),         # (c) N = 1024
    (64, 1025, 24000, 3),        # (c) N = 2048
    (258, 129, 200000, 3),       # (d) K = 4
    (33, 129, 5001, 7),          # (e) odd width, odd clip count, partial column tile (33 = 32 + 1)
    (40, 129, 100, 3),           # (f) the clip is shorter than one frame
    (20, 33, 3000, 3),           # N = 64: passes 8, 4
    (24, 65, 3000, 3),           # N = 128: passes 8, 8
    (16, 2049, 24000, 3),        # N = 4096: passes 8, 8, 8, 4; one frame per round
    (5, 129, 90000, 3),          # K = 71: a column's frames span several rounds
], ids=["b", "c1024", "c2048", "d", "e", "f", "n64", "n128", "n4096", "kbig"])
def test_shapes(gpu, width, height, n, n_clips):
    names = ("noise_full", "noise_33", "chirp")
    clips = np.stack([signal(names[i % 3], n, seed=i // 3) for i in range(n_clips)])
    check(render(clips, width, height), clips, width, height)


@pytest.mark.parametrize("range_db", [80.0, 120.0])
def test_g_dynamic_ranges(gpu, range_db):
    clip = signal("noise_33", A["n"])
    check(render(clip, A["width"], A["height"], range_db=range_db), [clip], A["width"], A["height"], range_db=range_db)


def test_top_db_shifts_the_scale(gpu):
    clip = signal("chirp", A["n"])
    check(render(clip, A["width"], A["height"], top_db=-6.0), [clip], A["width"], A["height"], top_db=-6.0)


def test_h_caller_supplied_dolph_window(gpu):
    w = sg.dolph(256, 100.0)
    clips = np.stack([signal(s, A["n"]) for s in ("noise_full", "chirp")])
    img = render(clips, A["width"], A["height"], window=w)
    check(img, clips, A["width"], A["height"], window=w)
    assert not np.array_equal(img, shape_a()[1][[0, 2]])          # (the table is used: the Hann image differs)


def test_one_clip_equals_the_same_clip_in_a_batch(gpu):
    clips, img = shape_a()
    for i in (0, 2, 5):
        assert np.array_equal(render(clips[i], A["width"], A["height"])[0], img[i])


def test_host_wrapper_equals_the_entry(gpu):
    clips, img = shape_a()
    assert np.array_equal(host.spectrogram(clips, RATE, A["width"]), img)


def device_render(data, f32, n_clips, n, width, height):
    d_in, d_img = _DevBuf(data.nbytes), _DevBuf(n_clips * height * width)
    try:
        d_in.upload(data)
        host.spectrogram_device(d_in.ptr, f32, n_clips, n, width, height, d_img.ptr)
        return d_img.download((n_clips, height, width), np.uint8)
    finally:
        d_in.free(); d_img.free()


def test_device_entry_with_int16_equals_the_host_entry(gpu):
    clips, img = shape_a()
    assert np.array_equal(device_render(clips, False, len(clips), A["n"], A["width"], A["height"]), img)


def test_resampled_path(gpu):
    n, width, height = 48000, 258, 129
    clips = np.stack([signal(s, n) for s in ("noise_full", "noise_33", "chirp", "tone")])
    one_call = render(clips, width, height, rate_in=48000, rate_out=24000)
    f32 = host.Resampler(48000, 24000).resample_f32(clips.astype(np.float32) / np.float32(32768.0))
    assert f32.dtype == np.float32 and f32.shape == (4, 24000)
    two_step = device_render(f32, True, 4, f32.shape[1], width, height)
    assert np.array_equal(one_call, two_step)
    for i in range(4):
        specref.compare(two_step[i], f32[i].astype(np.float64), width, height)
    # rate_out == rate_in renders at the source rate, like rate_out == 0
    assert np.array_equal(render(clips, width, height, rate_in=48000, rate_out=48000), render(clips, width, height, rate_in=48000))


def test_generate_batch_writes_the_wrapper_s_indices(gpu, tmp_path):
    clips = shape_a()[0][:3]
    paths = [str(tmp_path / f"clip{i}.png") for i in range(3)]
    for style, dyn in (("default", "100"), ("scientific", "80")):
        got = sg.generate_batch(clips, paths, 258, RATE, profile=sg.FrequencyProfile(0), style=style, dynamic_range=dyn)
        want = host.spectrogram(clips, RATE, 258, window=sg.style_window(style, 256, float(dyn)), range_db=float(dyn))
        assert np.array_equal(got, want)
        for i, p in enumerate(paths):
            idx, pal = decode_png(p)
            assert np.array_equal(idx, want[i]) and np.array_equal(pal, sg.palette(style))
    # the single-clip form, through the bird profile's resampler
    one = tmp_path / "one.png"
    sg.generate_from_pcm(clips[2].astype("<i2").tobytes(), str(one), 258, 48000)
    idx, _ = decode_png(one)
    assert np.array_equal(idx, host.spectrogram(clips[2], 48000, 258, rate_out=24000)[0])


# ---- the table caches hold 32 entries and the oldest leaves: 40 distinct keys evict and rebuild the first one
EVICT = dict(width=20, height=33, n=3000, keys=40)                # N = 64, the smallest legal transform


def evict_window(i):
    """Key i of 40: periodic Hann plus a small ramp of its own."""
    return specref.hann(64) + 1e-3 * (i + 1) * np.arange(64) / 64.0


def test_window_table_evicted_and_rebuilt(gpu):
    clip, W, H = signal("noise_33", EVICT["n"]), EVICT["width"], EVICT["height"]
    imgs = [render(clip, W, H, window=evict_window(i)) for i in range(EVICT["keys"])]
    assert not np.array_equal(imgs[0], imgs[39])
    assert np.array_equal(render(clip, W, H, window=evict_window(0)), imgs[0])
    check(imgs[39], [clip], W, H, window=evict_window(39))


def test_window_table_evicted_and_rebuilt_device_entry(gpu):
    clip, W, H, n = signal("noise_33", EVICT["n"]), EVICT["width"], EVICT["height"], EVICT["n"]
    d_in, d_img = _DevBuf(clip.nbytes), _DevBuf(H * W)
    try:
        d_in.upload(np.ascontiguousarray(clip))
        def go(i):
            host.spectrogram_device(d_in.ptr, False, 1, n, W, H, d_img.ptr, window=evict_window(i))
            return d_img.download((1, H, W), np.uint8)
        imgs = [go(i) for i in range(EVICT["keys"])]
        again = go(0)
    finally:
        d_in.free(); d_img.free()
    assert not np.array_equal(imgs[0], imgs[39])
    assert np.array_equal(again, imgs[0])
    check(imgs[39], [clip], W, H, window=evict_window(39))


def test_rate_table_evicted_and_rebuilt(gpu):
    """rate_in = 48000 + 100 i to 24000: L / M = 240 / (480 + i) in lowest terms; the largest phase table and span of the 40 (i = 37,
    L = 240, M = 517, T = 44) need 44 620 bytes of LDS, far below the limit, so every pair runs."""
    clip, W, H = signal("noise_33", EVICT["n"]), EVICT["width"], EVICT["height"]
    rates = [48000 + 100 * i for i in range(EVICT["keys"])]
    imgs = [render(clip, W, H, rate_in=r, rate_out=24000) for r in rates]
    assert not np.array_equal(imgs[0], imgs[39])
    assert np.array_equal(render(clip, W, H, rate_in=rates[0], rate_out=24000), imgs[0])
    f32 = host.Resampler(rates[39], 24000).resample_f32(clip.astype(np.float32)[None, :] / np.float32(32768.0))
    assert np.array_equal(imgs[39], device_render(f32, True, 1, f32.shape[1], W, H))
    specref.compare(imgs[39][0], f32[0].astype(np.float64), W, H)
