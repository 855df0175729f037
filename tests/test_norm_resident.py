"""k_clip_norm_resident: the plan's clip_minmax + normalize pair as ONE launch that keeps each clip in a CU's registers and LDS
between the min/max pass and the normalising pass (one read of the waveform instead of two).  min / max are exact whatever the
grouping and the four normalise operations are k_normalize's in its order, so nothing downstream may move by one bit: every case
compares the logits of an engine created with BNHIP_NORM_RESIDENT=1 against one created with =0 (the two launches) with
np.array_equal.  Which form a call really took is read from the per-step profile: the `normalize` step has a launch of its own
only when the pair ran."""
import ctypes as C

import numpy as np
import pytest

from birdnet_go_amd import host, synth_model as sm

pytestmark = pytest.mark.gpu


def _clips(n_clips, n_samples, rate):
    """Material, one all-zero clip (range 0: eps alone in the divisor), one clip whose extremes sit in its first and in its last
    quad (registers of thread 0 / the end of the LDS part at 144 000 samples, the partial last register round at 8 000)."""
    x = sm.synth_clips(n_clips, n_samples, rate, first=5)
    x[3] = 0.0
    peak = float(np.abs(x[7]).max())
    x[7, 1] = -1.5 * peak
    x[7, -2] = 1.75 * peak
    return x


class _DevBuf:
    """Device memory through the HIP runtime the library itself uses."""
    _hip = None

    def __init__(self, nbytes):
        if _DevBuf._hip is None:
            _DevBuf._hip = C.CDLL("libamdhip64.so")
        self.ptr = C.c_void_p()
        assert _DevBuf._hip.hipMalloc(C.byref(self.ptr), C.c_size_t(nbytes)) == 0

    def upload(self, arr):
        a = np.ascontiguousarray(arr)
        assert _DevBuf._hip.hipMemcpy(self.ptr, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0

    def download(self, shape):
        out = np.empty(shape, np.float32)
        assert _DevBuf._hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(out.nbytes), 2) == 0
        return out

    def at(self, byte_off):
        return self.ptr.value + byte_off

    def free(self):
        _DevBuf._hip.hipFree(self.ptr)


def _engine(blob, switch, monkeypatch, **kw):
    monkeypatch.setenv("BNHIP_NORM_RESIDENT", switch)          # read once, when the engine is built
    return host.HipClassifier(blob, autotune=False, **kw)


def _names_launched(c, call, kernel_class=None):
    """{step name: profile row} of the steps that had a launch of their own in `call`.  Unfiltered per-launch profiling runs the call
    on one lane and one context; filtered to one kernel class it leaves lanes and contexts as they run in production."""
    c.profile_filter(kernel_class)
    c.profile_enable(True)
    try:
        call()
        return {r["name"]: r for r in c.profile_read(per_step=True)[1]}
    finally:
        c.profile_enable(False)
        c.profile_filter(None)


def _both(blob, x, monkeypatch, max_batch, run=None, **kw):
    """{switch: logits} of the same call on an engine of each form, and the step names the switch-on engine launched."""
    n = x.shape[0]
    run = run or (lambda c: c.predict_batch(x.reshape(-1), n).copy())
    out, names = {}, None
    for switch in ("1", "0"):
        c = _engine(blob, switch, monkeypatch, max_batch=max_batch, **kw)
        try:
            out[switch] = run(c)
            if switch == "1":
                names = _names_launched(c, lambda: run(c))
        finally:
            c.close()
    assert np.isfinite(out["1"]).all()
    return out, names


def test_full_model_20_clips_bit_identical(gpu, full_blob, monkeypatch):
    """144 000 samples: 28 672 quads in registers, 7 328 in LDS; 20 clips is the smallest call above the 16-clip line."""
    x = _clips(20, 144000, 48000)
    out, names = _both(full_blob, x, monkeypatch, 20, lanes=1)
    assert "clip_minmax" in names and "normalize" not in names, list(names)[:4]
    assert names["clip_minmax"]["bytes"] == 20 * 144000 * 8, names["clip_minmax"]          # one read of x, one write of xn
    assert np.array_equal(out["1"], out["0"]), np.abs(out["1"] - out["0"]).max()
    assert np.abs(out["1"][3] - out["1"][0]).max() > 0          # (the silent clip is a clip of its own, not a copy)


def test_tiny_perch_registers_only(gpu, monkeypatch):
    """8 000 samples = 2 000 quads: registers only, the LDS part empty, the second register round partial, 26 rounds empty.  The
    Perch-style front-end feeds the raw clip to its STFT (no min/max, no normalise: nothing for the switch to change), so the
    config is taken once as it is and once with the v2.4 normalisation in front of the same log-mel layer, which has the pair."""
    x = _clips(20, 8000, 32000)
    out, names = _both(sm.build_model(sm.tiny_perch_config()), x, monkeypatch, 20, lanes=1)
    assert "clip_minmax" not in names and "normalize" not in names, list(names)[:4]
    assert np.array_equal(out["1"], out["0"])
    out, names = _both(sm.build_model(sm.tiny_perch_config(normalize=True)), x, monkeypatch, 20, lanes=1)
    assert "clip_minmax" in names and "normalize" not in names, list(names)[:4]
    assert np.array_equal(out["1"], out["0"]), np.abs(out["1"] - out["0"]).max()


def test_small_call_and_long_clip_keep_the_pair(gpu, full_blob, monkeypatch):
    """The fallback decision, not just the kernel: a 6-clip call keeps k_clip_minmax_parts + k_normalize, and a 160 000-sample clip
    (11 328 quads beyond the registers = 181 KB of LDS) does not fit on chip - both run the pair on a switch-on engine, same bits."""
    x = _clips(20, 144000, 48000)[2:8]
    out, names = _both(full_blob, x, monkeypatch, 20, lanes=1)
    assert "clip_minmax" in names and "normalize" in names, list(names)[:4]
    assert np.array_equal(out["1"], out["0"])
    long_blob = sm.build_model(sm.tiny_perch_config(n_samples=160000, normalize=True))
    xl = _clips(20, 160000, 32000)
    out, names = _both(long_blob, xl, monkeypatch, 20, lanes=1)
    assert "normalize" in names, list(names)[:4]
    assert np.array_equal(out["1"], out["0"])


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_pcm_entries_convert_in_the_launch(gpu, full_blob, monkeypatch, bits):
    """bnhip_predict_pcm16 / bnhip_predict_pcm: the PCM -> float32 conversion happens in the resident kernel's load (no float copy of
    the batch, no k_pcm*_to_f32 launch); equal to the switch-off engine, which converts first, and to the float entry fed the
    converted clips (sample / 2^15 at every depth: the 24- and 32-bit clips are the 16-bit ones shifted up)."""
    x = _clips(20, 144000, 48000)
    pcm = np.clip(np.round(x / np.abs(x).max() * 30000.0), -32768, 32767).astype(np.int16)
    if bits == 16:
        run = lambda c: c.predict_pcm16(pcm.reshape(-1), 20).copy()
    else:
        words = (pcm.astype(np.int64).reshape(-1) << (bits - 16)).astype("<i4")
        raw = words.tobytes() if bits == 32 else words.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
        run = lambda c: c.predict_pcm(raw, bits, 20).copy()
    out, names = _both(full_blob, pcm, monkeypatch, 20, run=run, lanes=1)
    assert "clip_minmax" in names and "normalize" not in names, list(names)[:4]
    # the launch read the PCM samples themselves and wrote xn: bits / 8 + 4 bytes per sample (a float copy first would make it 4 + 4)
    assert names["clip_minmax"]["launches"] == 1 and names["clip_minmax"]["bytes"] == 20 * 144000 * (bits // 8 + 4), names["clip_minmax"]
    assert np.array_equal(out["1"], out["0"]), np.abs(out["1"] - out["0"]).max()
    c = _engine(full_blob, "0", monkeypatch, max_batch=20, lanes=1)
    try:
        as_float = c.predict_batch((pcm.astype(np.float32) / np.float32(32768.0)).reshape(-1), 20)
    finally:
        c.close()
    assert np.array_equal(out["1"], as_float)


def test_depth_2_contexts_and_two_lanes(gpu, full_blob, monkeypatch):
    """Two calls in flight on a depth-2 engine (device pointers, one context each) and one 40-clip call split over two lanes of 20:
    every path goes through the same decision and equals the switch-off result."""
    x = _clips(40, 144000, 48000)
    nc = 6522

    def two_calls(c):
        xb, ob = _DevBuf(x.nbytes), _DevBuf(40 * nc * 4)
        try:
            xb.upload(x)
            for i in range(2):
                c.predict_device(xb.at(i * 20 * 144000 * 4), 20, ob.at(i * 20 * nc * 4))
            c.synchronize()
            return ob.download((40, nc)).copy()
        finally:
            xb.free(); ob.free()

    # which form ran is read from a profile filtered to the `frontend` class (normalize, melband), which leaves contexts and lanes as
    # they are: two launches of melband0+1 show that both contexts / both lanes were seen, normalize has two or none
    def front(c, call):
        rows = _names_launched(c, call, "frontend")
        return {k: r["launches"] for k, r in rows.items()}

    out, seen = {}, {}
    for switch in ("1", "0"):
        c = _engine(full_blob, switch, monkeypatch, max_batch=20, depth=2, lanes=1)
        try:
            out[switch] = two_calls(c)
            seen[switch] = front(c, lambda: two_calls(c))
        finally:
            c.close()
    assert seen["1"] == {"melband0+1": 2} and seen["0"] == {"normalize": 2, "melband0+1": 2}, seen
    assert np.isfinite(out["1"]).all() and np.array_equal(out["1"], out["0"])
    lanes, seen = {}, {}
    for switch in ("1", "0"):
        c = _engine(full_blob, switch, monkeypatch, max_batch=40, lanes=2)
        try:
            assert c.describe()["lanes"] == 2
            lanes[switch] = c.predict_batch(x.reshape(-1), 40).copy()
            seen[switch] = front(c, lambda: c.predict_batch(x.reshape(-1), 40))
        finally:
            c.close()
    assert seen["1"] == {"melband0+1": 2} and seen["0"] == {"normalize": 2, "melband0+1": 2}, seen
    assert np.isfinite(lanes["1"]).all() and np.array_equal(lanes["1"], lanes["0"])
