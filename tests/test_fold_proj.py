"""k_expand_dw_sk_proj: b1's narrow projection folded into b2's fused expand+depthwise launch.  The projection's f32-MFMA accumulator
(channels 4 kq .. + 3 of pixel li in lane (li, kq)) is the expand's resident operand, so the block prologue runs the projection - gate
multiply, k_pw_gemm's K order, bias afterwards - and the projection's launch and its output tensor disappear.  Every operation is the
pair's in its order: each case compares the logits of an engine created with BNHIP_FOLD_PROJ unset against one created with =0 with
np.array_equal.  Which form a call took is read from the per-step profile: `b1/project` has a launch of its own only when the pair ran.

Models: stem -> b1 -> b2 -> head.  The b2 input image is 27 x 75 (odd height, 14 x 38 outputs: a partial last tile in both directions,
tiles on all four image borders).  A call folds when it has at least half a block per CU (20 clips x >= 10 tiles against 256 CUs);
1- and 3-clip calls cut the chunk loop into parts and keep the pair.

The 8-channel b1: expdw_kw(8) = 8, so b2 runs k_expand_dw's half-slab form, not the chunk-loop form the fold exists for (its K order -
lane group kq holds k = 2 kq, + 1 - is not the accumulator's layout).  That model is not eligible by the form's own rule; the case
checks that it is left alone (the pair runs, same bits) and the padded N is covered by a 12-channel b1 (Kw = 16, rows 12 .. 15 zero)."""
import ctypes as C

import numpy as np
import pytest

from birdnet_go_amd import host, synth_model as sm

pytestmark = pytest.mark.gpu

N_SAMPLES = 512 + 94 * 149          # 150 frames
N_CLASSES = 50


def _cfg(stem, b1_out):
    return sm.tiny_config(n_samples=N_SAMPLES, n_mels=54, specs=(sm.SpecConfig(512, 94, 0.0, 3000.0), sm.SpecConfig(512, 94, 500.0, 15000.0)),
                          stem=stem, blocks=((1, 3, 1, b1_out, 1), (6, 3, 2, 24, 1)), top=64, n_classes=N_CLASSES)


_cache = {}


def _blob(stem, b1_out):
    if (stem, b1_out) not in _cache:
        _cache[(stem, b1_out)] = sm.build_model(_cfg(stem, b1_out))
    return _cache[(stem, b1_out)]


@pytest.fixture(scope="module")
def clips():
    return sm.synth_clips(40, N_SAMPLES, 48000, first=3)


def _engine(blob, switch, monkeypatch, **kw):
    if switch is None:
        monkeypatch.delenv("BNHIP_FOLD_PROJ", raising=False)
    else:
        monkeypatch.setenv("BNHIP_FOLD_PROJ", switch)          # read once, when the engine is built
    kw.setdefault("autotune", False)
    return host.HipClassifier(blob, **kw)


def _launched(c, call, kernel_class=None):
    c.profile_filter(kernel_class)
    c.profile_enable(True)
    try:
        call()
        return {r["name"]: r for r in c.profile_read(per_step=True)[1]}
    finally:
        c.profile_enable(False)
        c.profile_filter(None)


def _both(blob, monkeypatch, run, **kw):
    """{switch: logits} of the same call on a default engine and on a BNHIP_FOLD_PROJ=0 one, the steps the default engine launched
    and its describe()."""
    out, names, desc = {}, None, None
    for switch in (None, "0"):
        c = _engine(blob, switch, monkeypatch, **kw)
        try:
            out[switch] = run(c)
            if switch is None:
                names, desc = _launched(c, lambda: run(c)), c.describe()
        finally:
            c.close()
    assert np.isfinite(out[None]).all()
    return out, names, desc


def _assert_folded(names, desc, n):
    assert "b2/expand+dw" in names and "b1/project" not in names, sorted(names)
    # booked on b2's step with the bytes it moves: b1/project's input (and gate) in place of its output
    steps = {s["name"]: s for s in desc["steps"]}
    pj, ed = steps["b1/project"], steps["b2/expand+dw"]
    more = 4.0 * pj["H"] * pj["W"] * (pj["C"] - pj["Co"]) + (4.0 * pj["C"] if pj["fused_scale"] else 0.0)
    row = names["b2/expand+dw"]
    assert row["launches"] == 1 and more > 0
    # (the profile prints six significant digits; `more` is 2 % of the row)
    assert row["bytes"] == pytest.approx((ed["bytes"] + more) * n + ed["wbytes"], rel=1e-5), (row, ed, more)


@pytest.mark.parametrize("stem,b1_out", [(32, 16), (24, 16), (32, 12), (24, 12)])
def test_20_clips_fold_bit_identical(gpu, monkeypatch, clips, stem, b1_out):
    """Full and padded K (stem 32 / 24), full and padded N (16 / 12 channels): one launch, same bits."""
    x = clips[:20]
    out, names, desc = _both(_blob(stem, b1_out), monkeypatch, lambda c: c.predict_batch(x.reshape(-1), 20).copy(), max_batch=20, lanes=1)
    _assert_folded(names, desc, 20)
    assert np.array_equal(out[None], out["0"]), np.abs(out[None] - out["0"]).max()
    assert np.abs(out[None][1] - out[None][0]).max() > 0


def test_8_channel_b1_is_not_the_chunk_loop_form(gpu, monkeypatch, clips):
    """b1 with 8 output channels: b2's K is one half slab (k_expand_dw), the fold does not apply and the plan runs as before."""
    x = clips[:20]
    out, names, desc = _both(_blob(32, 8), monkeypatch, lambda c: c.predict_batch(x.reshape(-1), 20).copy(), max_batch=20, lanes=1)
    assert "b1/project" in names and "b2/expand+dw" in names, sorted(names)
    assert np.array_equal(out[None], out["0"])


@pytest.mark.parametrize("n", [1, 3])
def test_small_calls_keep_the_pair(gpu, monkeypatch, clips, n):
    """1 and 3 clips: the chunk loop is cut into parts over the CUs, the projection keeps its own launch - on the engine that folds
    its 20-clip calls - and a clip's bits do not depend on which form its call took."""
    x = clips[:20]
    c = _engine(_blob(32, 16), None, monkeypatch, max_batch=20, lanes=1)
    try:
        big = c.predict_batch(x.reshape(-1), 20).copy()
        small = c.predict_batch(x[:n].reshape(-1), n).copy()
        names = _launched(c, lambda: c.predict_batch(x[:n].reshape(-1), n))
    finally:
        c.close()
    assert "b1/project" in names and "b2/expand+dw" in names, sorted(names)
    assert np.array_equal(small, big[:n])
    c = _engine(_blob(32, 16), "0", monkeypatch, max_batch=20, lanes=1)
    try:
        assert np.array_equal(c.predict_batch(x[:n].reshape(-1), n), small)
    finally:
        c.close()


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


def test_40_clips_two_contexts_and_two_lanes(gpu, monkeypatch, clips):
    """40 clips as two 20-clip device calls in flight on a depth-2 engine, and as one call split over two lanes of 20.  A profile
    filtered to the pw_gemm class leaves contexts and lanes as they run: b1/project has no launch on the default engine, two on the
    switch-off one."""
    blob = _blob(32, 16)

    def two_calls(c):
        xb, ob = _DevBuf(clips.nbytes), _DevBuf(40 * N_CLASSES * 4)
        try:
            xb.upload(clips)
            for i in range(2):
                c.predict_device(xb.at(i * 20 * N_SAMPLES * 4), 20, ob.at(i * 20 * N_CLASSES * 4))
            c.synchronize()
            return ob.download((40, N_CLASSES)).copy()
        finally:
            xb.free(); ob.free()

    def projects(c, call):
        return {k: r["launches"] for k, r in _launched(c, call, "pw_gemm").items() if k in ("b1/project", "b2/project")}

    for kw, run in ((dict(max_batch=20, depth=2, lanes=1), two_calls), (dict(max_batch=40, lanes=2), lambda c: c.predict_batch(clips.reshape(-1), 40).copy())):
        out, seen = {}, {}
        for switch in (None, "0"):
            c = _engine(blob, switch, monkeypatch, **kw)
            try:
                out[switch] = run(c)
                seen[switch] = projects(c, lambda: run(c))
            finally:
                c.close()
        assert seen[None] == {"b2/project": 2} and seen["0"] == {"b1/project": 2, "b2/project": 2}, seen
        assert np.isfinite(out[None]).all() and np.array_equal(out[None], out["0"])


def test_pcm_entry_and_oracle_parity(gpu, monkeypatch, clips):
    """One call through the PCM entry (folded, equal to the switch-off engine), and the folded logits against the oracle."""
    from oracle.interp import Interpreter
    from test_parity_gpu import assert_parity
    blob = _blob(32, 16)
    x = clips[:20]
    pcm = np.clip(np.round(x / np.abs(x).max() * 30000.0), -32768, 32767).astype(np.int16)
    out, names, desc = _both(blob, monkeypatch, lambda c: c.predict_pcm16(pcm.reshape(-1), 20).copy(), max_batch=20, lanes=1)
    _assert_folded(names, desc, 20)
    assert np.array_equal(out[None], out["0"])
    c = _engine(blob, None, monkeypatch, max_batch=20, lanes=1)
    try:
        got = c.predict_batch(x.reshape(-1), 20).copy()
    finally:
        c.close()
    assert_parity(got[:3], Interpreter(blob).invoke(x[:3])[0])


def test_create_time_tuner_times_pair_against_fold(gpu, monkeypatch, clips):
    """An autotuned engine times the pair against the one launch on its own batch and keeps the faster; whichever it keeps, the
    logits are the switch-off engine's."""
    x = clips[:20]
    out, names, desc = _both(_blob(32, 16), monkeypatch, lambda c: c.predict_batch(x.reshape(-1), 20).copy(), max_batch=20, lanes=1, autotune=True)
    assert "b2/expand+dw" in names
    assert np.array_equal(out[None], out["0"])
