"""The plain depthwise, pooling and squeeze-excite kernels one level above tests/test_dwse_lab.py: through the planner.  Small graphs

    dw(k, s) -> SE (MEAN -> FC -> ReLU -> FC -> sigmoid -> MUL) -> 1 x 1 conv -> MEAN -> FC

whose FIRST layer is the depthwise under test, so that its input is the graph input and the lab's kernel-level gate applies, with the
oracle's own fp32 evaluation as err_f32:  err = max|got - ref64| / max|ref64| <= 4 err_f32 + 2^-22.  Fetched with debug_fetch and held
to the fp64 oracle: the depthwise step's output, the total of the slab sums its squeeze-excite block reads (per clip and channel:
pixels x (gate + 2^-24) in units of the output scale, as in the lab), and the squeeze-excite step's scale (the same gate on its own
scale).  This is where the slab count S that the planner (or, under BNHIP_DW_LDS, the tuner through set_sum_slabs) hands to the
consumers of the sums is checked, and where the planner's choice among k_dwconv_t, the LDS-staged form, k_dwconv<4> and k_dwconv<1>
is pinned per graph rather than left to the tuner of the day."""
import math

import numpy as np
import pytest

from birdnet_go_amd import host
from birdnet_go_amd import tflite_schema as S
from birdnet_go_amd.tflite_build import GraphBuilder
from oracle.interp import Interpreter

N_CLIPS = 3
ACTS = {"none": S.ACT_NONE, "relu": S.ACT_RELU, "relu6": S.ACT_RELU6}


def _graph(H, W, C, kh, kw, s, act, Cr=4, seed=11, lead=0):
    """-> (blob, tensors).  lead > 0: a 1 x 1 convolution from `lead` channels in front (the depthwise is then no longer the first layer)."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, np.float32)
    i32 = lambda a: np.asarray(a, np.int32)
    conv = lambda st, a: dict(padding=S.PAD_SAME, stride_w=st, stride_h=st, dilation_w_factor=1, dilation_h_factor=1, fused_activation_function=a)
    g = GraphBuilder(description="dw + se layer")
    x = t = g.tensor([1, H, W, lead or C], name="image")
    if lead:
        t = g.op("CONV_2D", [x, g.const(f32(rng.standard_normal((C, 1, 1, lead)) / np.sqrt(lead)), "lead/w"), g.const(f32(rng.standard_normal(C) * 0.1), "lead/b")],
                 [1, H, W, C], conv(1, S.ACT_RELU6), name="lead")
    Ho, Wo = math.ceil(H / s), math.ceil(W / s)
    gain = 3.0 if act == "relu6" else 1.0
    wd = f32(rng.standard_normal((1, kh, kw, C)) * gain / np.sqrt(kh * kw))
    bd = f32(rng.standard_normal(C) * 0.1 + (1.5 if act == "relu6" else 0.0))
    d = g.op("DEPTHWISE_CONV_2D", [t, g.const(wd, "dw/w"), g.const(bd, "dw/b")], [1, Ho, Wo, C],
             dict(conv(s, ACTS.get(act, S.ACT_NONE)), depth_multiplier=1), name="dw")
    if act == "swish":
        d = g.op("MUL", [d, g.op("LOGISTIC", [d], [1, Ho, Wo, C])], [1, Ho, Wo, C], {}, name="dw/swish")
    m = g.op("MEAN", [d, g.const(i32([1, 2]))], [1, C], dict(keep_dims=0), name="se/mean")
    r = g.op("FULLY_CONNECTED", [m, g.const(f32(rng.standard_normal((Cr, C)) / np.sqrt(C)), "se/w1"), g.const(f32(rng.standard_normal(Cr) * 0.1 + 0.3), "se/b1")],
             [1, Cr], dict(fused_activation_function=S.ACT_RELU), name="se/fc1")
    e = g.op("FULLY_CONNECTED", [r, g.const(f32(rng.standard_normal((C, Cr)) / np.sqrt(Cr)), "se/w2"), g.const(f32(rng.standard_normal(C) * 0.1), "se/b2")],
             [1, C], dict(fused_activation_function=S.ACT_NONE), name="se/fc2")
    sg = g.op("LOGISTIC", [e], [1, C], name="se/scale")
    sr = g.op("RESHAPE", [sg, g.const(i32([1, 1, 1, C]))], [1, 1, 1, C], dict(new_shape=[1, 1, 1, C]))
    u = g.op("MUL", [d, sr], [1, Ho, Wo, C], {}, name="se/mul")
    p = g.op("CONV_2D", [u, g.const(f32(rng.standard_normal((8, 1, 1, C)) / np.sqrt(C)), "proj/w"), g.const(f32(rng.standard_normal(8) * 0.1), "proj/b")],
             [1, Ho, Wo, 8], conv(1, S.ACT_NONE), name="proj")
    pm = g.op("MEAN", [p, g.const(i32([1, 2]))], [1, 8], dict(keep_dims=0), name="head/mean")
    y = g.op("FULLY_CONNECTED", [pm, g.const(f32(rng.standard_normal((5, 8)) / np.sqrt(8)), "head/w"), g.const(f32(np.zeros(5)), "head/b")], [1, 5],
             dict(fused_activation_function=S.ACT_NONE), name="head")
    return g.finish([x], [y]), dict(dw=d, scale=sg, Ho=Ho, Wo=Wo)


def _tiled_slabs(k, s, Ho, Wo, C):
    """dw_geometry of dwconv.hip restated: tiles of TH x TW outputs, PY = 256 / min(C / 4, 64) tiles (at most all of them) per slab."""
    TH, TW = {(3, 1): (2, 4), (3, 2): (2, 2), (5, 1): (2, 4), (5, 2): (1, 2)}[(k, s)]
    tiles = math.ceil(Wo / TW) * math.ceil(Ho / TH)
    PY = min(256 // min(C // 4, 64), tiles)
    return math.ceil(tiles / PY)


#           label            H   W   C  kh kw s  act      env                       kernel the depthwise step must take
VARIANTS = [("k3s1_tiled", 23, 21, 20, 3, 3, 1, "swish", {"BNHIP_NO_DW_LDS": "1"}, "tiled"),
            ("k5s2_tiled", 24, 23, 64, 5, 5, 2, "relu6", {"BNHIP_NO_DW_LDS": "1"}, "tiled"),
            ("k3s1_lds", 23, 21, 20, 3, 3, 1, "swish", {"BNHIP_DW_LDS": "1"}, "lds"),
            ("k5s2_lds", 24, 23, 64, 5, 5, 2, "relu6", {"BNHIP_DW_LDS": "1"}, "lds"),
            ("k3x1_generic4", 24, 24, 8, 3, 1, 1, "none", {}, "generic"),          # k_dwconv<4>, k_mean_partial with two pixel splits
            ("c6_generic1", 13, 11, 6, 3, 3, 1, "relu", {}, "generic")]            # k_dwconv<1>, scalar squeeze-excite, explicit MUL


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_depthwise_sums_and_scale_reproduce_the_f64_layer(gpu, monkeypatch, variant):
    label, H, W, C, kh, kw, s, act, env, form = variant
    blob, t = _graph(H, W, C, kh, kw, s, act)
    Ho, Wo = t["Ho"], t["Wo"]
    x = np.random.default_rng(5).standard_normal((N_CLIPS, H * W * C)).astype(np.float32)
    keep64, keep32 = {}, {}
    Interpreter(blob, "f64").invoke(x, keep=keep64)
    Interpreter(blob).invoke(x, keep=keep32)
    for k in ("BNHIP_NO_DW_LDS", "BNHIP_DW_LDS", "BNHIP_DW_PREFETCH", "BNHIP_SE_THREADS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    clf = host.HipClassifier(blob, max_batch=4, lanes=1, debug_no_reuse=True)
    try:
        steps = clf.describe()["steps"]
        clf.predict_batch(x.reshape(-1), N_CLIPS)
        dw = [q for q in steps if q["kernel"] == "dwconv"]
        se = [q for q in steps if q["kernel"] == "se"]
        assert len(dw) == 1 and len(se) == 1, [q["kernel"] for q in steps]
        dw, se = dw[0], se[0]
        assert dw["in_bf16"] == 0 and dw["out_bf16"] == 0
        if form == "generic":
            # no tiled kernel: no fused sums, a separate k_mean_partial over ceil(HW / 512) pixel splits feeds the squeeze-excite step
            assert dw["fused_sum"] == 0 and dw["dw_lds"] == 0
            mp = [q for q in steps if q["kernel"] == "mean" and q["name"] == "se/mean/partial"]
            assert len(mp) == 1 and mp[0]["S"] == se["S"] == math.ceil(Ho * Wo / 512) and (H != 24 or se["S"] == 2)
            sums_v, Sl = mp[0]["out_v"], se["S"]
        else:
            assert dw["fused_sum"] == 1 and dw["out2_v"] >= 0 and dw["dw_lds"] == (1 if form == "lds" else 0)
            assert se["S"] == dw["S"] >= 1                                      # the consumer follows the producer's slab count
            if form == "tiled":
                assert dw["S"] == _tiled_slabs(kh, s, Ho, Wo, C) and dw["S"] > 1
            sums_v, Sl = dw["out2_v"], dw["S"]
        # C % 4 == 0: the scale folds into the projection's operand load; otherwise an explicit MUL
        assert any(q["kernel"] == "elementwise" for q in steps) == (C % 4 != 0)
        assert any(q["fused_scale"] == 1 for q in steps) == (C % 4 == 0)

        ref = np.asarray(keep64[t["dw"]], np.float64).reshape(N_CLIPS, Ho * Wo, C)
        r32 = np.asarray(keep32[t["dw"]], np.float64).reshape(ref.shape)
        got = clf.debug_fetch(-2 - dw["out_v"], N_CLIPS, Ho * Wo * C).astype(np.float64).reshape(ref.shape)
        scale = float(np.abs(ref).max())
        err, e32 = float(np.abs(got - ref).max()) / scale, float(np.abs(r32 - ref).max()) / scale
        gate = 4 * e32 + 2.0 ** -22
        raw = clf.debug_fetch(-2 - sums_v, N_CLIPS, 64 * 64 * C).reshape(-1)
        sums = raw[:N_CLIPS * Sl * C].astype(np.float64).reshape(N_CLIPS, Sl, C).sum(axis=1)
        serr = float(np.abs(sums - ref.sum(axis=1)).max()) / scale
        sgate = Ho * Wo * (gate + 2.0 ** -24)
        sref = np.asarray(keep64[t["scale"]], np.float64).reshape(N_CLIPS, C)
        s32 = np.asarray(keep32[t["scale"]], np.float64).reshape(N_CLIPS, C)
        sgot = clf.debug_fetch(-2 - se["out_v"], N_CLIPS, C).astype(np.float64).reshape(N_CLIPS, C)
        sscale = float(np.abs(sref).max())
        cerr, c32 = float(np.abs(sgot - sref).max()) / sscale, float(np.abs(s32 - sref).max()) / sscale
        cgate = 4 * c32 + 2.0 ** -22
        print(f"{label}: y err {err:.3e} (fp32 oracle {e32:.3e}, gate {gate:.3e}); S = {Sl}, sums err {serr:.3e} of the y scale (gate {sgate:.3e}); "
              f"scale err {cerr:.3e} (fp32 oracle {c32:.3e}, gate {cgate:.3e}), scale range {sref.min():.3f} .. {sref.max():.3f}")
        assert np.isfinite(got).all() and err <= gate, (label, err, e32)
        assert np.isfinite(sums).all() and serr <= sgate, (label, serr, sgate)
        assert np.isfinite(sgot).all() and cerr <= cgate, (label, cerr, c32)
        assert sref.max() - sref.min() > 0.05                                     # a scale that depends on the sums
    finally:
        clf.close()


@pytest.mark.parametrize("kh,kw,C", [(3, 1, 8), (3, 3, 6)])
def test_generic_depthwise_steps_carry_no_bf16_storage(built_lib, kh, kw, C):
    """k_dwconv<VEC> reads and writes fp32 whatever DwParams::in_bf16 / out_bf16 say, so a step it will run must never be handed a bf16
    value: behind a 1 x 1 convolution and in front of one, on a "precision": "bf16" plan."""
    blob, _ = _graph(12, 12, C, kh, kw, 1, "none", lead=8)
    plan = host.HipClassifier(blob, plan_only=True, precision="bf16")
    try:
        d = plan.describe()
        dw = [q for q in d["steps"] if q["kernel"] == "dwconv"]
        assert d["precision"] == "bf16" and len(dw) == 1
        assert dw[0]["in_bf16"] == 0 and dw[0]["out_bf16"] == 0 and dw[0]["fused_sum"] == 0 and dw[0]["dw_lds"] == 0
    finally:
        plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kh,kw,C", [(3, 1, 8), (3, 3, 6)])
def test_generic_depthwise_steps_carry_no_bf16_storage_on_a_device_engine(gpu, kh, kw, C):
    """The same on a created engine (a plan-only engine marks no value as bf16 at all: the marking pass needs the tuned tiles)."""
    blob, _ = _graph(12, 12, C, kh, kw, 1, "none", lead=8)
    x = np.random.default_rng(6).standard_normal((N_CLIPS, 12 * 12 * 8)).astype(np.float32)
    clf = host.HipClassifier(blob, max_batch=4, lanes=1, precision="bf16")
    try:
        dw = [q for q in clf.describe()["steps"] if q["kernel"] == "dwconv"]
        assert len(dw) == 1 and dw[0]["in_bf16"] == 0 and dw[0]["out_bf16"] == 0
        got = clf.predict_batch(x.reshape(-1), N_CLIPS)
    finally:
        clf.close()
    ref = Interpreter(blob, "f64").invoke(x)[0]
    assert np.isfinite(got).all() and np.abs(got - ref).max() <= 0.05 * np.abs(ref).max()      # (bf16 GEMM operands: 2^-8 per product)


def _se_only(C, Cr):
    rng = np.random.default_rng(C)
    f32 = lambda a: np.asarray(a, np.float32)
    g = GraphBuilder(description="wide squeeze-excite")
    x = g.tensor([1, 2, 2, C], name="image")
    m = g.op("MEAN", [x, g.const(np.asarray([1, 2], np.int32))], [1, C], dict(keep_dims=0))
    r = g.op("FULLY_CONNECTED", [m, g.const(f32(rng.standard_normal((Cr, C)) / np.sqrt(C))), g.const(f32(np.zeros(Cr)))], [1, Cr], dict(fused_activation_function=S.ACT_RELU))
    e = g.op("FULLY_CONNECTED", [r, g.const(f32(rng.standard_normal((C, Cr)))), g.const(f32(np.zeros(C)))], [1, C], dict(fused_activation_function=S.ACT_NONE))
    sg = g.op("LOGISTIC", [e], [1, C])
    sr = g.op("RESHAPE", [sg, g.const(np.asarray([1, 1, 1, C], np.int32))], [1, 1, 1, C], dict(new_shape=[1, 1, 1, C]))
    u = g.op("MUL", [x, sr], [1, 2, 2, C], {})
    pm = g.op("MEAN", [u, g.const(np.asarray([1, 2], np.int32))], [1, C], dict(keep_dims=0))
    y = g.op("FULLY_CONNECTED", [pm, g.const(f32(rng.standard_normal((3, C)) / np.sqrt(C))), g.const(f32(np.zeros(3)))], [1, 3], dict(fused_activation_function=S.ACT_NONE))
    return g.finish([x], [y])


@pytest.mark.parametrize("C,Cr,fused", [(4100, 8, True), (12264, 8, True), (12268, 8, False), (12288, 64, False)])
def test_a_squeeze_excite_block_beyond_the_lds_limit_is_refused_at_plan_time(built_lib, C, Cr, fused):
    """k_se asks for (C + Cr + 4 * 1024 + 16) * 4 bytes of dynamic LDS at its largest block; a launch may ask for 64 KB.  Up to
    C + Cr = 12272 the planner builds the fused step; beyond, squeeze_excite refuses before it absorbs anything and the block runs on
    the generic steps (MEAN, two GEMMs, an elementwise MUL).  Plan only: nothing of that size is launched."""
    assert ((C + Cr + 4 * 1024 + 16) * 4 <= 64 * 1024) == fused
    plan = host.HipClassifier(_se_only(C, Cr), plan_only=True)
    try:
        kinds = [q["kernel"] for q in plan.describe()["steps"]]
    finally:
        plan.close()
    assert ("se" in kinds) == fused, kinds
    if not fused:
        assert "elementwise" in kinds and kinds.count("mean") >= 3, kinds          # the block's own MEAN (partial + finish) and the head's
