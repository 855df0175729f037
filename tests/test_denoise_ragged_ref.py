"""The ragged denoiser's bursts (tests/dnraggedcases.py) against the tie cap of the restatement, the documented workspace formula, and
every argument error of the five ragged C entries and of the Python surface's ragged / fused keywords, answered without a device
(ordinal 99).  CPU only."""
import ctypes as C
import math

import numpy as np
import pytest

import dnraggedcases as rc
import dnref
from birdnet_go_amd import host, process

INF = math.inf


@pytest.mark.parametrize("name", list(rc.BURSTS))
def test_tie_cap_holds_for_every_burst(name):
    """The cap is a condition on a burst's inputs, over its clips together: a burst that trips it gets another seed."""
    q, v = rc.restated(name)
    share = dnref.check_cap(v)
    print(f"{name}: {v.size} samples, excused share {share:.3g}")
    assert q.size == sum(rc.BURSTS[name][1])


@pytest.mark.parametrize("name", list(rc.BURSTS))
def test_workspace_size_is_the_documented_formula(built_lib, name):
    N, lens = rc.BURSTS[name]
    lib = host.load_library()
    arr = np.array(lens, np.int32)
    b = C.c_size_t(0)
    assert lib.bnhip_denoise_ragged_workspace_size(C.c_int(arr.size), C.c_void_p(arr.ctypes.data), C.c_int(N), C.byref(b)) == host.BNHIP_OK
    assert b.value == rc.workspace_formula(len(lens)) == host.denoise_ragged_workspace_size(lens, N)
    assert b.value % 256 == 0 and b.value >= 2 * (len(lens) + 1) * 8


def test_python_surface_refuses_before_any_device(built_lib, tmp_path):
    x = np.zeros((2, 100), np.int16)
    burst = [np.zeros(100, np.int16), np.zeros(57, np.int16)]
    paths = [str(tmp_path / "a.png"), str(tmp_path / "b.png")]
    for clips in (x, burst):
        with pytest.raises(ValueError, match="no filter active"):
            process.process_clips(clips, 24000, device=99, ragged=True)
        with pytest.raises(ValueError, match="no filter active"):
            process.processed_spectrogram(clips, paths, 64, 24000, device=99, fused=True)
        with pytest.raises(ValueError, match="denoise preset"):
            process.process_clips(clips, 24000, denoise="extreme", device=99, ragged=True)
        with pytest.raises(ValueError, match="denoise preset"):
            process.processed_spectrogram(clips, paths, 64, 24000, denoise="extreme", device=99, fused=True)
        with pytest.raises(ValueError, match="denoise preset"):
            process.denoise_clips(clips, 24000, preset="extreme", device=99, ragged=True)
        with pytest.raises(ValueError, match="gain_db"):
            process.process_clips(clips, 24000, gain_db=61.0, device=99, ragged=True)
        with pytest.raises(ValueError, match="gain_db"):
            process.processed_spectrogram(clips, paths, 64, 24000, gain_db=61.0, device=99, fused=True)
    with pytest.raises(ValueError, match="one output path per clip"):
        process.processed_spectrogram(burst, paths[:1], 64, 24000, denoise="medium", device=99, fused=True)
    with pytest.raises(ValueError, match="absolute"):
        process.processed_spectrogram(burst, ["a.png", "b.png"], 64, 24000, denoise="medium", device=99, fused=True)
    # unequal lengths need ragged=True / fused=True
    for call in (lambda: process.denoise_clips(burst, 24000, device=99), lambda: process.process_clips(burst, 24000, denoise="medium", device=99),
                 lambda: process.processed_spectrogram(burst, paths, 64, 24000, denoise="medium", device=99)):
        with pytest.raises((ValueError, host.HipError)):
            call()
    # mono int16 only
    for call in (lambda: host.denoise_ragged([c.astype(np.float32) for c in burst], 1024, 12, -40, device=99),
                 lambda: host.process_ragged([x], 24000, 1024, 12, -40, device=99),
                 lambda: process.denoise_clips([c.astype(np.int32) for c in burst], 24000, device=99, ragged=True)):
        with pytest.raises(host.HipError) as e:
            call()
        assert e.value.code == host.E_UNSUPPORTED
    with pytest.raises(host.HipError) as e:
        host.denoise_ragged([], 1024, 12, -40, device=99)
    assert e.value.code == host.E_INVALID


def test_argument_errors_need_no_device(built_lib):
    lib = host.load_library()
    ci, cd, vp, sz = C.c_int, C.c_double, C.c_void_p, C.c_size_t
    buf, out = np.zeros(4096, np.int16), np.zeros(4096, np.int16)
    res = (host.Loudness * 4)()
    good = np.array([1000, 24], np.int32)
    pal = np.zeros(768, np.uint8)
    height, _ = host.spectrogram_size(64)
    cap = host.png_max_bytes(2, 64, height)
    png = np.full(cap, 0x55, np.uint8)
    offs = np.zeros(3, np.uint64)
    p, o, r, ln = vp(buf.ctypes.data), vp(out.ctypes.data), vp(C.addressof(res)), vp(good.ctypes.data)
    dev = ci(99)
    err = lib.bnhip_last_error

    def size(n_clips=2, lens=ln, frame=256, dst=True):
        b = sz(0)
        return lib.bnhip_denoise_ragged_workspace_size(ci(n_clips), lens, ci(frame), C.byref(b) if dst else None)

    def pcm16(pcm=p, n_clips=2, lens=ln, frame=256, nr=12.0, nf=-40.0, dst=o):
        return lib.bnhip_denoise_ragged_pcm16(dev, pcm, ci(n_clips), lens, ci(frame), cd(nr), cd(nf), dst)

    def device(pcm=p, n_clips=2, lens=ln, frame=256, nr=12.0, nf=-40.0, dst=o, ws=r, ws_bytes=1 << 12):
        return lib.bnhip_denoise_ragged_device(dev, pcm, ci(n_clips), lens, ci(frame), cd(nr), cd(nf), dst, ws, sz(ws_bytes), vp())

    def chain(pcm=p, n_clips=2, lens=ln, rate=24000, frame=256, nr=12.0, nf=-40.0, normalize=1, t=-23.0, c=-2.0, gain=3.0, dst=o, rec=r):
        return lib.bnhip_process_ragged_pcm16(dev, pcm, ci(n_clips), lens, ci(rate), ci(frame), cd(nr), cd(nf), ci(normalize), cd(t), cd(c),
                                              cd(gain), dst, rec)

    def fused(pcm=p, n_clips=2, lens=ln, rate=24000, frame=256, nr=12.0, nf=-40.0, normalize=1, t=-23.0, c=-2.0, gain=3.0, rate_out=0,
              width=64, h=height, palette=vp(pal.ctypes.data), dst=vp(png.ctypes.data), out_cap=cap, off=vp(offs.ctypes.data), rec=r, pcm_out=vp()):
        return lib.bnhip_process_spectrogram_png_ragged_pcm16(dev, pcm, ci(n_clips), lens, ci(rate), ci(frame), cd(nr), cd(nf), ci(normalize),
                                                              cd(t), cd(c), cd(gain), ci(rate_out), ci(width), ci(h), vp(), cd(0.0), cd(100.0),
                                                              palette, dst, sz(out_cap), off, rec, pcm_out)

    zero = np.array([1000, 0], np.int32)
    # what all five share: the burst's lengths and the frame
    for fn in (size, pcm16, device, chain, fused):
        assert fn(lens=vp()) == host.E_INVALID and err() == b"NULL/empty argument", fn.__name__
        assert fn(lens=vp(zero.ctypes.data)) == host.E_INVALID and b"every clip length must be at least 1" in err(), fn.__name__
        for bad in (0, 65536):
            assert fn(n_clips=bad) == host.E_INVALID and b"n_clips" in err(), (fn.__name__, bad)
        for bad in (48, 32, 8192):
            assert fn(frame=bad) == host.E_INVALID and b"frame must be a power of two" in err(), (fn.__name__, bad)
    for fn in (size, pcm16, device):
        assert fn(frame=0) == host.E_INVALID and b"frame must be a power of two" in err()
    # what the four clip entries share
    for fn in (pcm16, device, chain, fused):
        assert fn(pcm=vp()) == host.E_INVALID and err() == b"NULL/empty argument", fn.__name__
        assert fn(dst=vp()) == host.E_INVALID and err() == b"NULL/empty argument", fn.__name__
        for bad in (math.nan, INF, -0.001, 97.001):
            assert fn(nr=bad) == host.E_INVALID and b"nr_db" in err(), (fn.__name__, bad)
        for bad in (math.nan, -INF, -80.001, -19.999):
            assert fn(nf=bad) == host.E_INVALID and b"nf_db" in err(), (fn.__name__, bad)
        # an acceptable call gets as far as the device: ordinal 99 does not exist (or there is no device at all)
        assert fn() in (host.E_INVALID, host.E_NO_DEVICE) and b"frame" not in err() and b"_db" not in err() and b"clip" not in err(), fn.__name__
    assert size() == host.BNHIP_OK and size(dst=False) == host.E_INVALID

    # the device entry: in and out must not overlap over the packed total (1024 samples), the workspace
    assert device(dst=p) == host.E_INVALID and b"must not overlap" in err()
    assert device(dst=vp(buf.ctypes.data + 2 * 1023)) == host.E_INVALID and b"must not overlap" in err()
    assert device(dst=vp(buf.ctypes.data + 2 * 1024)) in (host.E_INVALID, host.E_NO_DEVICE) and b"overlap" not in err()
    assert device(ws=vp()) == host.E_INVALID and err() == b"NULL/empty argument"
    assert device(ws_bytes=16) == host.E_INVALID and b"workspace smaller than bnhip_denoise_ragged_workspace_size" in err()

    # the two chains: the gain's range, no stage active, the records, the normalisation's own refusals
    for fn in (chain, fused):
        for bad in (math.nan, INF, 61.0, -60.001):
            assert fn(gain=bad) == host.E_INVALID and b"gain_db" in err(), (fn.__name__, bad)
        assert fn(frame=0, normalize=0, gain=0.0) == host.E_INVALID and b"no filter active" in err(), fn.__name__
        assert fn(rec=vp()) == host.E_INVALID and err() == b"NULL/empty argument", fn.__name__
        assert fn(rec=vp(), normalize=0) in (host.E_INVALID, host.E_NO_DEVICE) and err() != b"NULL/empty argument", fn.__name__
        assert fn(rate=7999) == host.E_INVALID and b"sample rate too low" in err(), fn.__name__
        assert fn(t=5.0) == host.E_INVALID and b"out of range" in err(), fn.__name__
        assert fn(c=1.0) == host.E_INVALID and b"must be <= 0" in err(), fn.__name__
        # frame 0 switches the denoiser off: its parameters are not looked at
        assert fn(frame=0, nr=math.nan, nf=0.0) in (host.E_INVALID, host.E_NO_DEVICE) and b"_db" not in err(), fn.__name__

    # the fused entry: the image, the palette, the offsets, the capacity - the output is not touched
    assert fused(out_cap=cap - 1) == host.E_INVALID and b"out_cap" in err()
    assert (png == 0x55).all()
    assert fused(palette=vp()) == host.E_INVALID and err() == b"NULL/empty argument"
    assert fused(off=vp()) == host.E_INVALID and err() == b"NULL/empty argument"
    assert fused(h=height + 1) == host.E_INVALID and b"height must be 2^k + 1" in err()
    assert fused(width=0) == host.E_INVALID and b"width" in err()
