"""The denoise spec's restatement (tests/dnref.py) against its own stated properties, on the signals of the GPU cases; the Python
surface's constants against ffmpeg/process.go:181-203; and every argument error of the four C entries, answered without a device
(ordinal 99).  CPU only."""
import ctypes as C
import math

import numpy as np
import pytest

import dncases
import dnref
from birdnet_go_amd import host, process

INF = math.inf


# ------------------------------------------------------------------------------------------------ the restatement's properties
@pytest.mark.parametrize("N,n", [(64, 7), (64, 1), (64, 5000), (256, 4099), (1024, dncases.PRESET_LEN), (4096, 10 * 4096 + 3)])
def test_identity_without_reduction(N, n):
    """nr_db = 0 makes every gain 1: analysis, synthesis and the 2/3 of the four Hann^2 windows give the input back."""
    for name in ("noise_full", "chirp", "tone_noise"):
        x = dncases.signal(name, n)
        v = dnref.denoise(x, N, 0.0, -40.0)
        assert np.abs(v - x).max() <= 1e-9, name
        assert np.array_equal(dnref.quant(v), x)


@pytest.mark.parametrize("preset", ["light", "medium"])
def test_a_clip_under_the_floor_leaves_at_the_gain_floor(preset):
    """Uniform noise in +-33 lies under both floors in every bin: every gain is g_min, so out = round(g_min pcm)."""
    nr, nf = dnref.PRESETS[preset]
    x = dncases.signal("noise_33", dncases.PRESET_LEN)
    q, v = dnref.denoise_pcm16(x, dncases.PRESET_N, nr, nf)
    want = dnref.g_min(nr) * x.astype(np.float64)
    assert np.abs(v[0] - want).max() <= 1e-9
    assert np.array_equal(q[0], dnref.quant(want))


def test_silence_stays_silent():
    for N, n in ((64, 7), (1024, dncases.PRESET_LEN)):
        v = dnref.denoise(np.zeros(n, np.int16), N, 20.0, -50.0)
        assert not v.any()


@pytest.mark.parametrize("case", list(dncases.CASES))
def test_tie_cap_holds_for_every_gpu_case(case):
    """The cap is a condition on a case's inputs: a case that trips it gets another seed."""
    _, v = dncases.restated(case)
    dnref.check_cap(v)


def test_noise_around_a_tone_drops():
    """A sanity bound only: the residual (output minus the clean tone) of tone_noise is smaller than the noise that went in."""
    n = dncases.PRESET_LEN
    x = dncases.signal("tone_noise", n).astype(np.float64)
    tone = np.round(8000.0 * np.sin(2.0 * np.pi * 1000.0 * np.arange(n) / dncases.RATE))
    noise_in = np.sqrt(np.mean((x - tone) ** 2))
    for preset in ("medium", "heavy"):
        v = dnref.denoise(x.astype(np.int16), dncases.PRESET_N, *dnref.PRESETS[preset])
        assert np.sqrt(np.mean((v - tone) ** 2)) < 0.8 * noise_in, preset


def test_quant_rounds_half_away_from_zero_and_saturates():
    v = np.array([0.5, -0.5, 1.5, -1.5, 0.49, 32767.4, 32767.5, 40000.0, -32768.5, -40000.0])
    assert dnref.quant(v).tolist() == [1, -1, 2, -2, 0, 32767, 32767, 32767, -32768, -32768]


# ------------------------------------------------------------------------------------------------ the Python surface's constants
def test_presets_and_validators_follow_the_reference():
    assert process.DENOISE_PRESETS == {"light": (6, -30), "medium": (12, -40), "heavy": (20, -50)} == dnref.PRESETS
    for p in ("", "light", "medium", "heavy"):
        assert process.is_valid_denoise_preset(p)
    for p in ("Light", "extreme", " ", "off"):
        assert not process.is_valid_denoise_preset(p)
    assert process.MAX_GAIN_DB == 60.0
    for g in (0, 0.0, -60.0, 60.0, 3.5):
        assert process.is_valid_gain_db(g)
    for g in (60.0001, -60.0001, math.nan, INF, -INF):
        assert not process.is_valid_gain_db(g)
    assert (process.LOUDNORM_TARGET_I, process.LOUDNORM_TARGET_TP) == (-23.0, -2.0)


def test_frame_for_rate():
    assert process.frame_for_rate(48000) == 2048
    assert process.frame_for_rate(32000) == 1024 and process.frame_for_rate(24000) == 1024
    assert process.frame_for_rate(8000) == 256 and process.frame_for_rate(16000) == 512
    assert process.frame_for_rate(1000) == 64 and process.frame_for_rate(384000) == 4096       # clamped
    with pytest.raises(ValueError):
        process.frame_for_rate(0)


def test_python_surface_refuses_before_any_device(built_lib):
    x = np.zeros((2, 100), np.int16)
    with pytest.raises(ValueError, match="no filter active"):
        process.process_clips(x, 24000, device=99)
    with pytest.raises(ValueError, match="no filter active"):
        process.processed_spectrogram(x, ["/tmp/a.png", "/tmp/b.png"], 64, 24000, device=99)
    with pytest.raises(ValueError, match="denoise preset"):
        process.process_clips(x, 24000, denoise="extreme", device=99)
    with pytest.raises(ValueError, match="denoise preset"):
        process.denoise_clips(x, 24000, preset="extreme", device=99)
    with pytest.raises(ValueError, match="gain_db"):
        process.process_clips(x, 24000, gain_db=61.0, device=99)
    for call in (lambda: host.denoise(x, 1024, 12, -40, channels=2, device=99), lambda: host.denoise(x.astype(np.float32), 1024, 12, -40, device=99),
                 lambda: host.process(x, 24000, 1024, 12, -40, channels=2, device=99), lambda: process.denoise_clips(x.astype(np.int32), 24000, device=99)):
        with pytest.raises(host.HipError) as e:
            call()
        assert e.value.code == host.E_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ the C entries' argument errors
def test_argument_errors_need_no_device(built_lib):
    lib = host.load_library()
    ci, cd, vp, sz = C.c_int, C.c_double, C.c_void_p, C.c_size_t
    buf = np.zeros(4096, np.int16)
    out = np.zeros(4096, np.int16)
    res = (host.Loudness * 4)()
    p, o, r = vp(buf.ctypes.data), vp(out.ctypes.data), vp(C.addressof(res))
    dev = ci(99)
    err = lib.bnhip_last_error

    def pcm16(pcm=p, n_clips=1, n=1024, frame=256, nr=12.0, nf=-40.0, dst=o):
        return lib.bnhip_denoise_pcm16(dev, pcm, ci(n_clips), ci(n), ci(frame), cd(nr), cd(nf), dst)

    def device(pcm=p, n_clips=1, n=1024, frame=256, nr=12.0, nf=-40.0, dst=o, ws=r, ws_bytes=1 << 12):
        return lib.bnhip_denoise_device(dev, pcm, ci(n_clips), ci(n), ci(frame), cd(nr), cd(nf), dst, ws, sz(ws_bytes), vp())

    def chain(pcm=p, n_clips=1, n=1024, rate=24000, frame=256, nr=12.0, nf=-40.0, normalize=1, t=-23.0, c=-2.0, gain=3.0, dst=o, rec=r):
        return lib.bnhip_process_pcm16(dev, pcm, ci(n_clips), ci(n), ci(rate), ci(frame), cd(nr), cd(nf), ci(normalize), cd(t), cd(c), cd(gain),
                                       dst, rec)

    def size(n_clips=1, n=1024, frame=256, dst=True):
        b = sz(0)
        return lib.bnhip_denoise_workspace_size(ci(n_clips), ci(n), ci(frame), C.byref(b) if dst else None)

    # what the three clip entries share
    for fn in (pcm16, device, chain):
        assert fn(pcm=vp()) == host.E_INVALID and err() == b"NULL/empty argument", fn.__name__
        assert fn(dst=vp()) == host.E_INVALID and err() == b"NULL/empty argument", fn.__name__
        for bad in (0, -1, 65536):
            assert fn(n_clips=bad) == host.E_INVALID and b"n_clips" in err(), fn.__name__
        for bad in (0, -5):
            assert fn(n=bad) == host.E_INVALID and b"n must be" in err(), fn.__name__
        for bad in (-256, 1, 32, 63, 96, 1000, 4097, 8192):
            assert fn(frame=bad) == host.E_INVALID and b"frame must be a power of two" in err(), (fn.__name__, bad)
        for bad in (math.nan, INF, -INF, -0.001, 97.001):
            assert fn(nr=bad) == host.E_INVALID and b"nr_db" in err(), (fn.__name__, bad)
        for bad in (math.nan, INF, -INF, -80.001, -19.999, 0.0):
            assert fn(nf=bad) == host.E_INVALID and b"nf_db" in err(), (fn.__name__, bad)
    for fn in (pcm16, device):
        assert fn(frame=0) == host.E_INVALID and b"frame must be a power of two" in err()
    # an acceptable call gets as far as the device: ordinal 99 does not exist (or there is no device at all)
    for fn in (pcm16, device, chain):
        assert fn() in (host.E_INVALID, host.E_NO_DEVICE) and b"frame" not in err() and b"_db" not in err(), fn.__name__
    for frame in (64, 128, 4096):
        assert size(frame=frame) == host.BNHIP_OK

    # the device entry: in and out must not overlap, the workspace
    assert device(dst=p) == host.E_INVALID and b"must not overlap" in err()
    assert device(dst=vp(buf.ctypes.data + 2 * 1000)) == host.E_INVALID and b"must not overlap" in err()
    assert device(ws=vp()) == host.E_INVALID and err() == b"NULL/empty argument"
    assert device(ws_bytes=16) == host.E_INVALID and b"workspace smaller than bnhip_denoise_workspace_size" in err()
    need = host.denoise_workspace_size(3, 5000, 64)
    assert need >= 1 and need % 256 == 0
    assert size(dst=False) == host.E_INVALID
    assert size(n_clips=0) == host.E_INVALID and size(n=0) == host.E_INVALID and size(frame=100) == host.E_INVALID

    # the chain: the gain's range (IsValidGainDB), no stage active, the normalisation's own refusals, the records
    for bad in (math.nan, INF, -INF, 60.001, -60.001):
        assert chain(gain=bad) == host.E_INVALID and b"gain_db" in err(), bad
    assert chain(frame=0, normalize=0, gain=0.0) == host.E_INVALID and b"no filter active" in err()
    assert chain(rec=vp()) == host.E_INVALID and err() == b"NULL/empty argument"
    assert chain(rec=vp(), normalize=0) in (host.E_INVALID, host.E_NO_DEVICE) and err() != b"NULL/empty argument"
    assert chain(rate=7999) == host.E_INVALID and b"sample rate too low" in err()
    assert chain(rate=7999, normalize=0) in (host.E_INVALID, host.E_NO_DEVICE) and b"sample rate" not in err()
    assert chain(t=5.0) == host.E_INVALID and b"out of range" in err()
    assert chain(c=1.0) == host.E_INVALID and b"must be <= 0" in err()
    # frame 0 switches the denoiser off: its parameters are not looked at
    assert chain(frame=0, nr=math.nan, nf=0.0) in (host.E_INVALID, host.E_NO_DEVICE) and b"_db" not in err()
