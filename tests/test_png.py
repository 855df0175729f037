"""PNG on the device (bnhip_png_*, bnhip_spectrogram_png_pcm16) against the restatement of the spec (tests/pngref.py) and an
independent reader (tests/pngdec.py).

Acceptance: the encoder is integer arithmetic, so every byte and every offset equals the restatement's; the reader returns the image
and the palette; the device entry equals the host entry; the fused entry equals bnhip_spectrogram_pcm16 followed by
bnhip_png_encode_u8.  The cases (tests/pngcases.py) are images of a few KB; those with several bands are narrow and tall, since a
band that is not the last holds at least 16384 bytes."""
import ctypes as C

import numpy as np
import pytest

import pngcases as K
import pngdec
import pngref
from birdnet_go_amd import host, spectrogram as sg

from test_flac import first_difference
from test_parity_gpu import _DevBuf
from test_spectrogram import A, RATE, shape_a, signal

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", K.NAMES)
def test_bytes_and_offsets_equal_the_restatement(gpu, name):
    images, _ = K.cases()[name]
    want, want_off = K.reference(name)
    got, off = host.png_encode(images, K.palette(), raw=True)
    assert off.tolist() == want_off.tolist(), name
    assert got.tobytes() == want, (name, first_difference(got.tobytes(), want))
    assert int(off[-1]) <= host.png_max_bytes(*images.shape[:1], images.shape[2], images.shape[1])
    for i in range(0, len(images), max(1, len(images) // 4)):          # (the restatement's own streams decode in test_png_ref.py)
        idx, pal = pngdec.decode(got[int(off[i]):int(off[i + 1])].tobytes())
        assert np.array_equal(idx, images[i]) and np.array_equal(pal, K.palette()), (name, i)


def test_batch_offsets_are_the_running_sum(gpu):
    images, _ = K.cases()["batch300"]
    streams = host.png_encode(images, K.palette())
    _, off = host.png_encode(images, K.palette(), raw=True)
    assert len(streams) == 300 and off.tolist() == np.concatenate(([0], np.cumsum([len(s) for s in streams]))).tolist()
    assert len({len(s) for s in streams[0::3]}) == 1 and len({len(s) for s in streams[2::3]}) == 1      # ZERO and STORED have one size
    # an image's stream does not depend on its neighbours
    for i in (0, 1, 2, 299):
        assert host.png_encode(images[i], K.palette())[0] == streams[i]


def device_encode(images, pal, cap=None, ws=None):
    n, h, w = images.shape
    cap = host.png_max_bytes(n, w, h) if cap is None else cap
    ws = host.png_workspace_size(n, w, h) if ws is None else ws
    bufs = d_in, d_out, d_off, d_ws = _DevBuf(images.nbytes), _DevBuf(cap), _DevBuf(8 * (n + 1)), _DevBuf(max(ws, 256))
    try:
        d_in.upload(images)
        host.png_encode_device(d_in.ptr, n, w, h, pal, d_out.ptr, cap, d_off.ptr, d_ws.ptr, ws)
        off = d_off.download((n + 1,), np.uint64)                        # (a blocking copy on the null stream: after the kernels)
        return d_out.download((cap,), np.uint8)[:int(off[-1])], off
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("name", ["1x1", "zero_between", "stored_both", "three_images", "batch300"])
def test_device_entry_equals_the_host_entry(gpu, name):
    images, _ = K.cases()[name]
    want, want_off = host.png_encode(images, K.palette(), raw=True)
    got, off = device_encode(images, K.palette())
    assert off.tolist() == want_off.tolist() and got.tobytes() == want.tobytes()


def test_one_byte_short_is_invalid(gpu):
    images, _ = K.cases()["three_images"]
    n, h, w = images.shape
    cap, ws = host.png_max_bytes(n, w, h), host.png_workspace_size(n, w, h)
    for kw, word in ((dict(cap=cap - 1), "out_cap"), (dict(ws=ws - 1), "workspace")):
        with pytest.raises(host.HipError) as e:
            device_encode(images, K.palette(), **kw)
        assert e.value.code == host.E_INVALID and word in str(e.value)
    lib = host.load_library()
    out, off = np.zeros(cap, np.uint8), np.zeros(n + 1, np.uint64)
    lib.bnhip_png_encode_u8.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    pal = np.ascontiguousarray(K.palette()).reshape(-1)
    assert lib.bnhip_png_encode_u8(0, images.ctypes.data, n, w, h, pal.ctypes.data, out.ctypes.data, cap - 1, off.ctypes.data) == host.E_INVALID
    assert lib.bnhip_png_encode_u8(0, images.ctypes.data, n, w, h, pal.ctypes.data, out.ctypes.data, cap, off.ctypes.data) == host.BNHIP_OK


def test_fused_entry_equals_render_then_encode(gpu):
    clips, img = shape_a()
    pal = sg.palette("default")
    streams = host.spectrogram_png(clips, RATE, A["width"], pal)
    assert streams == host.png_encode(img, pal)
    assert streams == [pngref.encode(im, pal) for im in img]
    for s, im in zip(streams, img):
        idx, p = pngdec.decode(s)
        assert np.array_equal(idx, im) and np.array_equal(p, pal)


def test_fused_entry_equals_render_then_encode_resampled(gpu):
    n = 48000
    clips = np.stack([signal(s, n) for s in ("noise_full", "noise_33", "chirp", "silence")])
    pal = sg.palette("scientific")
    w = sg.dolph(256, 100.0)
    img = host.spectrogram(clips, 48000, A["width"], rate_out=24000, window=w, range_db=80.0)
    got = host.spectrogram_png(clips, 48000, A["width"], pal, rate_out=24000, window=w, range_db=80.0)
    assert got == host.png_encode(img, pal)
    assert not img[3].any() and np.array_equal(pngdec.decode(got[3])[0], img[3])


def test_generate_batch_writes_the_device_s_stream(gpu, tmp_path):
    clips = shape_a()[0][:3]
    paths = [str(tmp_path / f"clip{i}.png") for i in range(3)]
    dev_paths = [str(tmp_path / f"dev{i}.png") for i in range(3)]
    for style, dyn in (("default", "100"), ("scientific", "80")):
        want = sg.generate_batch(clips, paths, 258, RATE, profile=sg.FrequencyProfile(0), style=style, dynamic_range=dyn)
        got = sg.generate_batch(clips, dev_paths, 258, RATE, profile=sg.FrequencyProfile(0), style=style, dynamic_range=dyn, device_png=True)
        assert np.array_equal(got, want)
        for i, p in enumerate(dev_paths):
            data = open(p, "rb").read()
            idx, pal = pngdec.decode(data)
            assert np.array_equal(idx, want[i]) and np.array_equal(pal, sg.palette(style))
            assert data == pngref.encode(want[i], sg.palette(style))
    one = tmp_path / "one.png"
    sg.generate_from_pcm(clips[2].astype("<i2").tobytes(), str(one), 258, 48000, device_png=True)
    assert np.array_equal(pngdec.decode(open(one, "rb").read())[0], host.spectrogram(clips[2], 48000, 258, rate_out=24000)[0])
