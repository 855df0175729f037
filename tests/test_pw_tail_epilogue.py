"""The fused tails of the split-bf16 GEMM (k_pw_b16 with clip-aligned row tiles, pw_b16.hip): an expand whose only reader is a stride-1
SAME 3 x 3 / 5 x 5 depthwise convolution runs that convolution and its squeeze-excite sums in its epilogue, the layer in front of the
global pooling writes the pooled vector.  BNHIP_PW_TAIL=2 takes the fused form wherever the plan marks a step, =0 nowhere.

The fused kernels repeat the operation order of the launches they replace (k_dwconv_t, k_mean_partial + k_mean_finish), so every
comparison between the two switches here is BIT FOR BIT - no tolerance of its own.  The one comparison against the fp64 oracle uses the
gate of tests/test_expdw_layers.py (err <= 4 * err_f32 + 2^-16 on the layer's output scale; the sums: times the pixels summed)."""
import ctypes

import numpy as np
import pytest

from birdnet_go_amd import host, synth_model as sm
from oracle.interp import Interpreter
from oracle.tflite_reader import read_model

FORMS = [(13, 6), (14, 6), (15, 6), (14, 4), (13, 8)]       # (PwParams::wm = 48- / 96- / 192-row tiles, 16-column units)
CALLS = (1, 3, 5)                                           # a partial first block and a ragged last one for tiles of 2 and 4 clips
MAXB = 8


def _tail_cfg(n_mels, frames):
    """Four halvings (stem + three stride-2 blocks): 48 x 256 -> a 3 x 16 tail, 32 x 128 -> 2 x 8.  The last stage has 136 input
    channels (> 128: expand and depthwise stay two steps), 816 expanded channels (no multiple of 64, 96 or 128: a column tail), one
    5 x 5 and one 3 x 3 stride-1 block, and a top of 200 columns (no multiple of a column tile either)."""
    hop = 94
    specs = (sm.SpecConfig(512, hop, 0.0, 3000.0), sm.SpecConfig(512, hop, 500.0, 15000.0))
    return sm.tiny_config(n_samples=512 + hop * (frames - 1), n_mels=n_mels, specs=specs, stem=8,
                          blocks=((1, 3, 1, 8, 1), (6, 3, 2, 12, 1), (6, 5, 2, 20, 1), (6, 5, 2, 136, 2), (6, 3, 1, 136, 1)),
                          top=200, n_classes=50, emit_embeddings=True, seed=4242, name="tail_synth")


MODELS = {"A": (48, 256, 3, 16), "B": (32, 128, 2, 8)}


@pytest.fixture(scope="module")
def tail_models():
    out = {}
    for label, (n_mels, frames, H, W) in MODELS.items():
        cfg = _tail_cfg(n_mels, frames)
        out[label] = (cfg, sm.build_model(cfg), sm.synth_clips(max(CALLS), cfg.n_samples, cfg.sample_rate, first=5))
    return out


def _steps(blob, **kw):
    c = host.HipClassifier(blob, plan_only=True, **kw)
    try:
        return c.describe()["steps"]
    finally:
        c.close()


def _marked(steps):
    return {s["name"].split("+")[0]: s["tail"] for s in steps if s["tail"]}


# ------------------------------------------------------------------------------------------------ plan only (no GPU)
def test_plan_marks_the_stride1_tail_pairs_and_the_pooled_top(built_lib, full_blob, monkeypatch):
    """v2.4 stack: the 192 -> 1152 expands of b13 - b16 (more than 128 input channels: expand and depthwise are two steps) in front of
    their stride-1 depthwise convolutions at 3 x 16, and `top` in front of the pooling - and nothing else."""
    monkeypatch.delenv("BNHIP_PW_TAIL", raising=False)
    steps = _steps(full_blob)
    assert _marked(steps) == {"b13/expand": 2, "b14/expand": 2, "b15/expand": 2, "b16/expand": 2, "top": 1}
    for i, s in enumerate(steps):
        if s["tail"] == 2:
            d = steps[i + 1]
            assert d["kernel"] == "dwconv" and d["stride"] == 1 and d["k"] in (3, 5) and (d["H"], d["W"]) == (3, 16) and s["Co"] == 1152
        if s["tail"] == 1:
            assert [t["kernel"] for t in steps[i + 1:i + 3]] == ["mean", "mean"] and (s["H"], s["W"]) == (3, 16)
    assert not any(s["absorbed"] for s in steps)             # marked, not taken: that is the tuner's decision


def test_switch_off_is_todays_plan(built_lib, full_blob, monkeypatch):
    monkeypatch.delenv("BNHIP_PW_TAIL", raising=False)
    plain = _steps(full_blob)
    monkeypatch.setenv("BNHIP_PW_TAIL", "0")
    off = _steps(full_blob)
    assert not _marked(off)
    strip = lambda steps: [{k: v for k, v in s.items() if k != "tail"} for s in steps]
    assert strip(off) == strip(plain)                        # marking alone changes no tile, name, flop or byte figure
    assert [s["name"] for s in off] == [s["name"] for s in plain] and len(off) == 61


def test_tail_without_a_clip_aligned_tile_stays_unfused(built_lib, monkeypatch):
    """5 x 20 = 100 pixels per clip: no multiple of 16, no row tile of whole clips - even when forced."""
    monkeypatch.setenv("BNHIP_PW_TAIL", "2")
    cfg = _tail_cfg(80, 320)
    steps = _steps(sm.build_model(cfg))
    tail = [s for s in steps if s["kernel"] == "dwconv" and s["C"] == 816]
    assert len(tail) == 2 and all((s["H"], s["W"]) == (5, 20) for s in tail)
    assert not _marked(steps) and all(s["wm"] < 13 and s["wm_full"] < 13 for s in steps)


def test_fused_step_reports_both_halves(built_lib, tail_models, monkeypatch):
    """(describe() prints six significant digits: sums of printed figures agree to 1e-5 relative.)"""
    near = lambda v: pytest.approx(v, rel=1e-5)
    cfg, blob, _ = tail_models["A"]
    monkeypatch.setenv("BNHIP_PW_TAIL", "0")
    off = _steps(blob, max_batch=MAXB)
    monkeypatch.setenv("BNHIP_PW_TAIL", "2")
    on = _steps(blob, max_batch=MAXB)
    assert len(on) == len(off)
    fused = [i for i, s in enumerate(on) if s["tail"]]
    assert [on[i]["tail"] for i in fused] == [2, 2, 1]
    for i in fused:
        n = 1 if on[i]["tail"] == 2 else 2
        assert on[i]["kernel"] == "pw_gemm" and on[i]["wm_full"] >= 13
        assert on[i]["name"] == off[i]["name"] + ("+dw" if n == 1 else "+mean")
        assert on[i]["flops"] == near(sum(off[j]["flops"] for j in range(i, i + n + 1)))
        assert all(on[j]["absorbed"] == 1 and on[j]["flops"] == 0 and on[j]["bytes"] == 0 for j in range(i + 1, i + n + 1))
        # bytes really moved: the GEMM's own output stays on chip (depthwise: replaced by the depthwise output, the same size)
        gone = 4.0 * on[i]["H"] * on[i]["W"] * on[i]["Co"]
        assert on[i]["bytes"] == near(off[i]["bytes"] if n == 1 else off[i]["bytes"] - gone + 4.0 * on[i]["Co"])
    assert sum(s["flops"] for s in on) == near(sum(s["flops"] for s in off))


# ------------------------------------------------------------------------------------------------ on the GPU
def _tail_launches():
    lib = host.load_library()
    lib.bnhip_debug_pw_tail_launches.restype = ctypes.c_long
    return lib.bnhip_debug_pw_tail_launches()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(blob, x, n, **kw):
    """One serial engine, one call of n clips: logits, embeddings (= the pooled vector), and per depthwise step of the tail its
    output tensor, its squeeze-excite partial sums and the expanded tensor's slot."""
    clf = host.HipClassifier(blob, max_batch=MAXB, lanes=1, debug_no_reuse=True, **kw)
    try:
        steps = clf.describe()["steps"]
        before = _tail_launches()
        logits, emb = clf.predict_batch(x[:n].reshape(-1), n, want_embeddings=True)
        used = _tail_launches() - before
        layers = {}
        for i, s in enumerate(steps):
            if s["kernel"] == "dwconv" and s["C"] == 816:
                HW, C = s["H"] * s["W"], s["C"]
                y = clf.debug_fetch(-2 - s["out_v"], n, HW * C)
                sums = clf.debug_fetch(-2 - s["out2_v"], n, 64 * C)
                ex = clf.debug_fetch(-2 - steps[i - 1]["out_v"], n, HW * C)
                layers[s["name"]] = (y.copy(), sums.copy(), ex.copy())
        return dict(logits=logits.copy(), emb=emb.copy(), layers=layers, used=used, steps=steps)
    finally:
        clf.close()


@pytest.fixture(scope="module")
def unfused(gpu, tail_models):
    """The reference side of every comparison, computed once: BNHIP_PW_TAIL=0, tuners off (the plan's default tiles)."""
    mp = pytest.MonkeyPatch()
    mp.setenv("BNHIP_PW_TAIL", "0")
    try:
        out = {(label, n): _run(blob, x, n, autotune=0) for label, (cfg, blob, x) in tail_models.items() for n in CALLS}
    finally:
        mp.undo()
    assert all(r["used"] == 0 for r in out.values())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f"wm{f[0]}nt{f[1]}")
@pytest.mark.parametrize("label", ["A", "B"])
def test_fused_equals_unfused_bit_for_bit(gpu, tail_models, unfused, monkeypatch, label, form):
    cfg, blob, x = tail_models[label]
    H, W = MODELS[label][2:]
    monkeypatch.setenv("BNHIP_PW_TAIL", "2")
    monkeypatch.setenv("BNHIP_PW_TAIL_FORM", f"{form[0]},{form[1]}")
    one = {}
    for n in CALLS:
        got, ref = _run(blob, x, n, autotune=0), unfused[(label, n)]
        marked = [s for s in got["steps"] if s["tail"]]
        assert [(s["tail"], s["wm_full"], s["nt_full"]) for s in marked] == [(2, *form), (2, *form), (1, *form)], (label, form)
        assert got["used"] == 3, "the fused kernel ran for both depthwise pairs and the pooled top"
        assert len(got["layers"]) == 2 and sorted(s["k"] for s in got["steps"] if s["kernel"] == "dwconv" and s["C"] == 816) == [3, 5]
        for name, (y, sums, ex) in got["layers"].items():
            ry, rsums, _ = ref["layers"][name]
            assert next(s["dw_lds"] for s in got["steps"] if s["name"] == name) == 0      # the register-tiled kernel's sums
            tiles = -(-H // 2) * -(-W // 4)                  # dw_geometry: tiles of 2 x 4 outputs, PY = min(256 / 64, tiles) of them per chunk
            slabs = -(-tiles // min(4, tiles))
            assert slabs == {"A": 2, "B": 1}[label]
            k = n * slabs * 816                              # partial[b][chunk][c], packed
            assert np.array_equal(_bits(y), _bits(ry)), (label, form, n, name, "depthwise output")
            assert np.array_equal(_bits(sums.reshape(-1)[:k]), _bits(rsums.reshape(-1)[:k])), (label, form, n, name, "squeeze-excite sums")
            assert np.abs(sums.reshape(-1)[:k]).min() > 0
            assert np.isfinite(y).all() and np.abs(y).max() > 0
        assert np.array_equal(_bits(got["emb"]), _bits(ref["emb"])), (label, form, n, "pooled vector")
        assert np.array_equal(_bits(got["logits"]), _bits(ref["logits"])), (label, form, n, "logits")
        assert got["emb"].shape == (n, 200) and np.abs(got["emb"]).max() > 0
        one[n] = got["logits"]
    # a clip's logits do not depend on the size of the call it arrives in
    assert np.array_equal(_bits(one[1][0]), _bits(one[5][0])) and np.array_equal(_bits(one[3]), _bits(one[5][:3]))


@pytest.mark.gpu
def test_fused_run_never_writes_the_expanded_tensor(gpu, tail_models, monkeypatch):
    """The absorbed value keeps its arena slot (small calls of a tuned engine run the pair); a fused call must leave it alone: with every
    value in a buffer of its own, the slot holds the same words after calls on different clips - and not the expanded tensor."""
    cfg, blob, x = tail_models["A"]
    monkeypatch.setenv("BNHIP_PW_TAIL", "0")
    ref = _run(blob, x, 3, autotune=0)
    monkeypatch.setenv("BNHIP_PW_TAIL", "2")
    clf = host.HipClassifier(blob, max_batch=MAXB, lanes=1, debug_no_reuse=True, autotune=0)
    try:
        steps = clf.describe()["steps"]
        slots = [s for s in steps if s["tail"] == 2]
        assert len(slots) == 2
        seen = []
        for first in (0, 2):
            clf.predict_batch(x[first:first + 3].reshape(-1), 3)
            seen.append([_bits(clf.debug_fetch(-2 - s["out_v"], 3, 48 * 816)).copy() for s in slots])
        for a, b, s in zip(seen[0], seen[1], slots):
            assert np.array_equal(a, b), s["name"]
            assert not np.array_equal(a, _bits(ref["layers"][s["name"].split("+")[0].replace("expand", "dw")][2])), s["name"]
    finally:
        clf.close()


def _swish_out(m, t):
    for lg in m.ops:
        if lg.name == "LOGISTIC" and list(lg.inputs) == [t]:
            for mu in m.ops:
                if mu.name == "MUL" and sorted(mu.inputs) == sorted([t, lg.outputs[0]]):
                    return mu.outputs[0]
    return t


@pytest.mark.gpu
def test_fused_layers_against_the_f64_oracle(gpu, tail_models, monkeypatch):
    """The gate of tests/test_expdw_layers.py on the fused steps' own outputs: err = max|got - ref64| / max|ref64| <= 4 * err_f32 + 2^-16,
    err_f32 the fp32 oracle's error on the same tensor; the sums: the same bound times the pixels summed, plus fp32 accumulation."""
    cfg, blob, x = tail_models["A"]
    n = 3
    m = read_model(blob)
    keep64, keep32 = {}, {}
    Interpreter(m, "f64").invoke(x[:n], keep=keep64)
    Interpreter(m).invoke(x[:n], keep=keep32)
    monkeypatch.setenv("BNHIP_PW_TAIL", "2")
    got = _run(blob, x, n, autotune=0)
    assert got["used"] == 3
    for name, (y, sums, _) in got["layers"].items():
        dw = next(o for o in m.ops if o.name == "DEPTHWISE_CONV_2D" and m.tensors[o.outputs[0]].name == name)
        ti = _swish_out(m, dw.outputs[0])
        ref = np.asarray(keep64[ti], np.float64).reshape(n, 48, 816)
        r32 = np.asarray(keep32[ti], np.float64).reshape(ref.shape)
        scale = float(np.abs(ref).max())
        err = float(np.abs(y.astype(np.float64).reshape(ref.shape) - ref).max()) / scale
        e32 = float(np.abs(r32 - ref).max()) / scale
        gate = 4 * e32 + 2.0 ** -16
        s = sums.reshape(-1)[:n * 2 * 816].astype(np.float64).reshape(n, 2, 816).sum(axis=1)
        serr = float(np.abs(s - ref.sum(axis=1)).max()) / scale
        sgate = 48 * (gate + 2.0 ** -24)
        print(f"{name}: y err {err:.3e} (fp32 oracle {e32:.3e}, gate {gate:.3e}); sums err {serr:.3e} (gate {sgate:.3e})")
        assert err <= gate and serr <= sgate, (name, err, gate, serr, sgate)
    # the pooled vector: the mean of `top`'s output over the 48 pixels, behind the whole stack - the logits' own parity gate
    ref_logits = Interpreter(m).invoke(x[:n])[0]
    assert (got["logits"].argmax(1) == ref_logits.argmax(1)).all()
    sig = lambda v: 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))
    assert np.abs(sig(got["logits"]) - sig(ref_logits)).max() <= 1e-4


class _DevBuf:
    """Device memory through the HIP runtime the library itself uses."""
    _hip = None

    def __init__(self, nbytes):
        if _DevBuf._hip is None:
            _DevBuf._hip = ctypes.CDLL("libamdhip64.so")
        self.ptr = ctypes.c_void_p()
        assert _DevBuf._hip.hipMalloc(ctypes.byref(self.ptr), ctypes.c_size_t(nbytes)) == 0

    def upload(self, arr):
        a = np.ascontiguousarray(arr)
        assert _DevBuf._hip.hipMemcpy(self.ptr, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.nbytes), 1) == 0

    def download(self, shape):
        out = np.empty(shape, np.float32)
        assert _DevBuf._hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), self.ptr, ctypes.c_size_t(out.nbytes), 2) == 0
        return out

    def at(self, off):
        return self.ptr.value + off

    def free(self):
        _DevBuf._hip.hipFree(self.ptr)


def _pipelined(blob, x, calls, **kw):
    """The calls, back to back, through a depth-2 engine: successive device calls alternate between the two contexts (own stream, own
    arena).  Returns logits [call][clip] and the number of fused launches."""
    clf = host.HipClassifier(blob, max_batch=MAXB, depth=2, lanes=1, **kw)
    nc = 50
    xd, out = _DevBuf(x.nbytes), _DevBuf(len(calls) * 5 * nc * 4)
    try:
        steps = clf.describe()["steps"]
        xd.upload(x)
        before = _tail_launches()
        for call, n in enumerate(calls):
            clf.predict_device(xd.at(0), n, out.at(call * 5 * nc * 4))
        clf.synchronize()
        return out.download((len(calls), 5, nc)), _tail_launches() - before, steps
    finally:
        clf.close()
        xd.free(); out.free()


@pytest.mark.gpu
@pytest.mark.parametrize("label", ["A", "B"])
def test_fused_on_both_contexts_of_a_pipelined_engine(gpu, tail_models, monkeypatch, label):
    """(A pipelined call runs the squeeze-excite kernel with other workgroups than a serial one - another fixed summation order - so the
    reference here is the unfused depth-2 engine.)"""
    cfg, blob, x = tail_models[label]
    calls = (5, 5, 3, 1)                                          # contexts 0, 1, 0, 1
    monkeypatch.setenv("BNHIP_PW_TAIL", "0")
    ref, used0, _ = _pipelined(blob, x, calls, autotune=0)
    monkeypatch.setenv("BNHIP_PW_TAIL", "2")
    got, used, steps = _pipelined(blob, x, calls, autotune=0)
    assert used0 == 0 and used == 3 * len(calls)
    assert [s["tail"] for s in steps if s["tail"]] == [2, 2, 1]
    for call, n in enumerate(calls):
        assert np.array_equal(_bits(got[call, :n]), _bits(ref[call, :n])), (label, call, n)
        assert np.array_equal(_bits(got[call, :n]), _bits(got[0, :n]))        # neither the context nor the call's size shows in a clip's logits
    assert np.abs(got[0]).max() > 0


@pytest.mark.gpu
def test_forced_tuner_picks_a_fused_form_per_layer(gpu, tail_models, monkeypatch):
    """Tuners on, forced: autotune_tail times every fused candidate and keeps the fastest (its choice is a timing: only that it is a
    fused form, that it ran, and the result are checked - the logits under the parity gate of tests/test_parity_gpu.py, since the other
    layers' tuned tiles differ from an untuned engine's)."""
    cfg, blob, x = tail_models["A"]
    monkeypatch.setenv("BNHIP_PW_TAIL", "2")
    got = _run(blob, x, 5)
    marked = [s for s in got["steps"] if s["tail"]]
    assert len(marked) == 3 and all(s["wm_full"] in (13, 14, 15) and s["nt_full"] in (4, 6, 8) and s["wm"] >= 13 for s in marked)
    assert got["used"] == 3
    ref = Interpreter(blob).invoke(x[:5])[0]
    sig = lambda v: 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))
    assert (got["logits"].argmax(1) == ref.argmax(1)).all() and np.abs(sig(got["logits"]) - sig(ref)).max() <= 1e-4
