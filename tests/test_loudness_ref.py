"""Clip loudness on the CPU: the restatement (tests/loudref.py) against the reference's own known answers and tolerances, the
distance between the float64 spec and the float32 restatement of the Go meter, the host arithmetic of birdnet_go_amd.loudness, and
the C ABI's argument errors (answered before any device is touched)."""
import ctypes as C
import math

import numpy as np
import pytest

import birdnet_go_amd  # noqa: F401
from birdnet_go_amd import host, loudness

import loudref as R

INF = math.inf
FS = 48000


def noise_int16(seed, n, amp):
    return np.clip(np.round(np.random.default_rng(seed).standard_normal(n) * amp * 32768.0), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def kats():
    """Every signal measured once, in both modes: name -> (int16 clip, spec measurement, go32 measurement)."""
    tone = R.sine_int16(-23, 1000, 4, FS)
    # (the two gating cases keep the reference's durations - a block that straddles the edge passes the relative gate, so a
    # shorter tone would move the answer - and run at 8 kHz, where 1 kHz is as flat in the K-weighting, to keep the loops short)
    tone8 = R.sine_int16(-23, 1000, 10, 8000)
    sig = {
        "tone": (tone, FS),                                                                                    # meter_test.go:64-70
        "tone8": (tone8, 8000),
        "tone_silence": (np.concatenate([tone8, np.zeros(80000, np.int16)]), 8000),                             # :51-60
        "loud_quiet": (np.concatenate([R.sine_int16(-20, 1000, 5, 8000), R.sine_int16(-50, 1000, 5, 8000)]), 8000),   # :131-139
        "short": (R.sine_int16(-23, 1000, 0.2, FS), FS),                                                       # :142-147
        "peak6": (R.sine_int16(-6, 1000, 1, FS), FS),                                                          # truepeak_test.go
        "peak3_5k": (R.sine_int16(-3, 5000, 0.5, FS), FS),
        "zeros": (np.zeros(FS, np.int16), FS),
        "noise": (np.concatenate([noise_int16(1, FS, 0.1), noise_int16(2, FS // 2, 0.002), noise_int16(3, FS, 0.1)]), FS),
        "modulated": ((noise_int16(4, 2 * FS, 0.2).astype(np.float64)
                       * (0.55 + 0.45 * np.sin(2 * np.pi * 1.3 * np.arange(2 * FS) / FS))).astype(np.int16), FS),
        "tone_11k": (R.sine_int16(-30, 440, 2, 11025), 11025),
    }
    return {k: (v, R.measure(v, rate), R.measure(v, rate, go32=True)) for k, (v, rate) in sig.items()}


MONO = 10.0 * math.log10(2.0)      # one channel of the reference's stereo test tones


@pytest.mark.parametrize("mode", [1, 2])
def test_reference_known_answers(kats, mode):
    m = {k: v[mode] for k, v in kats.items()}
    assert abs(m["tone"]["L"] - (-23.0 - MONO)) <= 0.1
    assert abs(m["tone8"]["L"] - (-23.0 - MONO)) <= 0.1
    assert abs(m["tone_silence"]["L"] - m["tone8"]["L"]) <= 0.1         # the silence is gated: unchanged
    assert abs(m["tone_silence"]["L"] - (-23.0 - MONO)) <= 0.1
    assert abs(m["loud_quiet"]["L"] - (-20.0 - MONO)) <= 0.2            # the quiet half is relative-gated
    assert m["short"]["L"] == -INF
    assert abs(m["peak6"]["dbtp"] - (-6.0)) <= 0.2
    assert m["zeros"]["dbtp"] == -INF and m["zeros"]["L"] == -INF and m["zeros"]["P"] == 0.0
    for k, (s, _, _) in kats.items():
        assert m[k]["P"] >= float(np.max(np.abs(s.astype(np.float64)))) / 32768.0, k


def test_spec_is_within_the_reference_float32_figure_of_the_go_restatement(kats):
    """1e-3 LU is meter.go:38-39's own figure for float32 against float64; a float32 32-tap sum is bounded near 3.5e-5 dB, so
    1e-3 dBTP also covers the reference's unpinned SIMD order."""
    dl = dp = 0.0
    for k, (_, a, b) in kats.items():
        assert (a["L"] == -INF) == (b["L"] == -INF), k
        if a["L"] != -INF:
            dl = max(dl, abs(a["L"] - b["L"]))
        if a["P"] > 0:
            dp = max(dp, abs(a["dbtp"] - b["dbtp"]))
    print(f"spec vs go32: loudness {dl:.3e} LU, true peak {dp:.3e} dB")
    assert dl <= 1e-3 and dp <= 1e-3


def test_sub_block_is_go_round():
    assert [R.sub_block(r) for r in (8000, 11025, 44100, 48000, 256000)] == [800, 1103, 4410, 4800, 25600]
    assert host.loudness_sub_block(11025) == 1103 and round(0.1 * 11025) == 1102


def test_k_weighting_coefficients_at_48k():
    want = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
            1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]                       # kweight_test.go
    assert np.abs(np.array(R.kweight64(48000)) - want).max() <= 1e-6
    assert all(float(np.float32(c)) == c for c in R.kweight(48000))


def test_true_peak_taps_are_a_partition_of_unity():
    c = R.tp_coef64()
    assert c.shape == (4, 32) and np.abs(c.sum(1) - 1.0).max() <= 1e-15
    assert np.allclose(c[0], c[3][::-1], rtol=0, atol=1e-15) and np.allclose(c[1], c[2][::-1], rtol=0, atol=1e-15)


def test_plan_gain_and_clamp_cases():
    o = loudness.Options(-3.0, -6.0)
    p = loudness.plan_gain(-10.0, -10.0, o)                                  # TestNormalizePeakLimited: +7 wanted, +4 allowed
    assert (p.target_gain_db, p.gain_db, p.peak_limited, p.output_lufs) == (7.0, 4.0, True, -6.0)
    p = loudness.plan_gain(-INF, -INF)                                       # TestNormalizeSilenceIsNoOp
    assert (p.gain_db, p.output_lufs, p.peak_limited) == (0.0, -INF, False)
    p = loudness.plan_gain(-30.0, -INF)
    assert (p.gain_db, p.peak_limited) == (7.0, False)
    assert loudness.default_options() == loudness.Options(-23.0, -1.0)
    assert (loudness.DEFAULT_MAX_GAIN_DB, loudness.EXPORT_MAX_GAIN_DB) == (30.0, 60.0)
    M = 30.0
    for gain, lim, want in [(12.5, M, (12.5, False)), (M, M, (M, False)), (M + 5, M, (M, True)), (-M, M, (-M, False)),        # TestClampGainDB
                            (-M - 5, M, (-M, True)), (0, M, (0, False)), (50, -M, (M, True)), (-50, -M, (-M, True)), (10, -M, (10, False)),
                            (500.0, INF, (500.0, False))]:
        assert loudness.clamp_gain_db(gain, lim) == want
        assert R.plan_gain(-INF, -10.0, -23.0, -2.0) == (0.0, 0.0, False)
    assert loudness.factor_from_db(0.0) == 1.0 and loudness.factor_from_db(-0.0) == 1.0
    assert loudness.factor_from_db(20.0) == 10.0 and loudness.factor_from_db(-6.0) == math.pow(10.0, -0.3)


def test_gate_fallback_cases():
    """TestGateFallbackGainDB (native_normalization_test.go:170-227): target -23, ceiling -2."""
    tiny = np.array([3, -3] * 4800, np.int16)
    r = R.normalize(tiny, 8000, -23.0, -2.0, 60.0, gate_fallback=True)
    assert r["integrated_lufs"] == -INF and r["flags"] & R.GATE_LIFTED
    assert abs(r["lift_db"] - 47.0) <= 1e-9                                 # flat clip: bounded by target + 70, not by 78 dB of headroom
    sil = R.normalize(np.zeros(9600, np.int16), 8000, -23.0, -2.0, 60.0, gate_fallback=True)
    assert sil["flags"] == 0 and sil["gain_db"] == 0.0 and sil["factor"] == 1.0          # digital silence is left alone
    loud = R.normalize(R.sine_int16(-30, 440, 1.2, 8000), 8000, -23.0, -2.0, 60.0, gate_fallback=True)
    assert not loud["flags"] & R.GATE_LIFTED                                # measurable: PlanGain's business
    peaky = np.zeros(9600, np.int16)
    peaky[4000] = 200                                                       # one -44 dBFS click: loudness under the gate
    r = R.normalize(peaky, 8000, -23.0, -2.0, 60.0, gate_fallback=True)
    assert r["integrated_lufs"] == -INF and abs(r["lift_db"] - (-2.0 - r["true_peak_dbtp"])) <= 1e-12 and r["lift_db"] < 47.0


def test_pcmgain_rounds_half_away_and_saturates():
    s = np.array([1, -1, 3, -3, 32767, -32768, 0, 101], np.int16)
    assert R.apply_gain(s, 0.5).tolist() == [1, -1, 2, -2, 16384, -16384, 0, 51]
    assert R.apply_gain(s, 2.0).tolist() == [2, -2, 6, -6, 32767, -32768, 0, 202]
    assert R.apply_gain(s, 1.0).tolist() == s.tolist()
    assert R.round_half_away(np.array([0.49999999999999994, -0.49999999999999994, 2.5, -2.5])).tolist() == [0.0, -0.0, 3.0, -3.0]


# ---------------------------------------------------------------------------------------------------- C ABI, no device needed
ENTRIES = ("bnhip_loudness_measure_pcm16", "bnhip_loudness_normalize_pcm16", "bnhip_loudness_workspace_size", "bnhip_loudness_normalize_device")


def test_loudness_symbols_are_exported(built_lib):
    lib = host.load_library()
    for s in ENTRIES:
        assert s in host.SYMBOLS and getattr(lib, s)
    assert C.sizeof(host.Loudness) == 80


def test_go_shim_restates_the_record_and_binds_both_entries():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    body = lambda src: re.sub(r"\s+", " ", re.search(r"typedef struct bnhip_loudness \{(.*?)\} bnhip_loudness;", src, flags=re.S).group(1)).strip()
    shim_dir = os.path.join(root, "birdnet-go_amd", "go", "internal", "inference", "hip")
    shim = open(os.path.join(shim_dir, "backend_hip.go")).read()
    stub = open(os.path.join(shim_dir, "stub_nohip.go")).read()
    assert body(shim) == body(open(os.path.join(root, "include", "bnhip.h")).read())
    assert '"bnhip_loudness_measure_pcm16"' in shim and '"bnhip_loudness_normalize_pcm16"' in shim
    for src in (shim, stub):
        assert "type Loudness struct" in src and "type LoudnessOptions struct" in src
    for fn in ("func MeasureLoudness(pcm []int16, nClips, sampleRate, device int) ([]Loudness, error)",
               "func NormalizeClips(pcm []int16, nClips, sampleRate int, opts LoudnessOptions, device int) (out []int16, res []Loudness, err error)"):
        b = shim[shim.index(fn):]
        b = b[:b.index("\n}\n")]
        assert "runtime.LockOSThread()" in b and "defer runtime.UnlockOSThread()" in b, fn
    assert "func MeasureLoudness([]int16, int, int, int) ([]Loudness, error)" in stub
    assert "func NormalizeClips([]int16, int, int, LoudnessOptions, int) ([]int16, []Loudness, error)" in stub


def test_loudness_argument_errors_before_any_device(built_lib):
    lib = host.load_library()
    ci, cd, vp = C.c_int, C.c_double, C.c_void_p
    buf = np.zeros(4096, np.int16)
    out = (host.Loudness * 4)()
    p, o = vp(buf.ctypes.data), vp(C.addressof(out))
    dev = ci(99)                                                             # no such device: a valid call would fail differently

    def measure(pcm=p, n_clips=1, n=1024, rate=48000, res=o):
        return lib.bnhip_loudness_measure_pcm16(dev, pcm, ci(n_clips), ci(n), ci(rate), res, vp())

    def norm(pcm=p, n_clips=1, n=1024, rate=48000, t=-23.0, c=-1.0, g=30.0, res=o):
        return lib.bnhip_loudness_normalize_pcm16(dev, pcm, ci(n_clips), ci(n), ci(rate), cd(t), cd(c), cd(g), ci(1), vp(), res)

    def device(pcm=p, n_clips=1, n=1024, rate=48000, t=-23.0, c=-1.0, g=30.0, res=o, ws=p, ws_bytes=1 << 20):
        return lib.bnhip_loudness_normalize_device(dev, pcm, ci(n_clips), ci(n), ci(rate), cd(t), cd(c), cd(g), ci(0), vp(), res, ws,
                                                   C.c_size_t(ws_bytes), vp())

    for fn in (measure, norm, device):
        assert fn(pcm=vp()) == host.E_INVALID and lib.bnhip_last_error() == b"NULL/empty argument"
        assert fn(res=vp()) == host.E_INVALID
        for bad in (0, -1, 65536):
            assert fn(n_clips=bad) == host.E_INVALID and b"n_clips" in lib.bnhip_last_error()
        assert fn(n=0) == host.E_INVALID and b"n must be" in lib.bnhip_last_error()
        for bad in (0, 4, 7999):                                             # TestNormalizeValidation, TestMeasureRejectsTooLowSampleRate
            assert fn(rate=bad) == host.E_INVALID and b"sample rate too low" in lib.bnhip_last_error()
    for fn in (norm, device):
        for bad in (math.nan, INF, -INF):
            assert fn(t=bad) == host.E_INVALID and b"target loudness must be finite" in lib.bnhip_last_error()
        for bad in (5.0, 0.0, -70.0, -80.0):
            assert fn(t=bad) == host.E_INVALID and b"out of range" in lib.bnhip_last_error()
        for bad in (math.nan, INF, -INF):
            assert fn(c=bad) == host.E_INVALID and b"ceiling must be finite" in lib.bnhip_last_error()
        assert fn(c=1.0) == host.E_INVALID and b"must be <= 0" in lib.bnhip_last_error()
        assert fn(g=math.nan) == host.E_INVALID and b"max_gain_db" in lib.bnhip_last_error()
    assert device(ws=vp()) == host.E_INVALID
    assert device(ws_bytes=16) == host.E_INVALID and b"workspace" in lib.bnhip_last_error()
    need = C.c_size_t(0)
    assert lib.bnhip_loudness_workspace_size(ci(3), ci(48000), ci(48000), C.byref(need)) == host.BNHIP_OK and need.value > 0
    assert host.loudness_workspace_size(3, 48000, 48000) == need.value
    assert lib.bnhip_loudness_workspace_size(ci(3), ci(48000), ci(48000), None) == host.E_INVALID
    assert lib.bnhip_loudness_workspace_size(ci(3), ci(48000), ci(100), C.byref(need)) == host.E_INVALID


def test_only_mono_int16_is_supported(built_lib):
    for call in (lambda: host.loudness_measure(np.zeros(100, np.int16), 48000, channels=2),
                 lambda: host.loudness_normalize(np.zeros(100, np.int16), 48000, channels=2),
                 lambda: host.loudness_measure(np.zeros(100, np.float32), 48000),
                 lambda: loudness.normalize_clips([np.zeros((50, 2), np.int16)], 48000)):
        with pytest.raises(host.HipError) as e:
            call()
        assert e.value.code == host.E_UNSUPPORTED
