"""The pointwise / dense GEMM kernels one level above tests/test_pw64_lab.py: through the planner.  Small graphs go through the planner
with autotune=False, lanes=1 (the planner's own tile, shrunk by pw_fill_grid for a call of three clips: what a Predict of a few
clips runs); every GEMM step's output is fetched with debug_fetch and held to the fp64 oracle's tensor under the layer tests' gate

    err = max|got - ref64| / max|ref64| <= 4 err_f32oracle + 2^-16

(the 2^-16 is for the layers behind the first, whose input already carries the error of the layers in front).  On the one-product
engine ("precision": "bf16") the operands are rounded to bf16, so the oracle of the whole graph is no reference for a layer: there each
step is held to fp64 RE-EVALUATED on that step's own inputs as fetched from the device, rounded as the kernel rounds them (a scale
multiplied in fp32, then RNE to bf16; weights RNE to bf16), under the lab's gate 4 err_f32host + 2^-22, plus one bf16 ulp of the
element where the step stores bf16.  describe() pins which kernel family and row tile every step was planned on."""
import numpy as np
import pytest

from birdnet_go_amd import host
from birdnet_go_amd import tflite_schema as S
from birdnet_go_amd.tflite_build import GraphBuilder
from oracle.interp import Interpreter

N_CLIPS = 3
f32 = lambda a: np.ascontiguousarray(a, np.float32)
i32 = lambda a: np.asarray(a, np.int32)


def bf16_round(a):
    """Round to nearest even to bf16, as v_cvt_pk_bf16_f32 does; returned widened to float32."""
    u = f32(a).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16 << 16).astype(np.uint32).view(np.float32).reshape(np.shape(a))


def dense_stack():
    """FULLY_CONNECTED 100 -> 72 -> 20 -> 36 -> 9: K tails of 4, 8 and 20 columns inside the last slab, and one slab exactly (K = 36: 4)."""
    rng = np.random.default_rng(21)
    g = GraphBuilder(description="dense stack")
    x = t = g.tensor([1, 100], name="features")
    layers, dims = [], [100, 72, 20, 36, 9]
    for li in range(4):
        K, N = dims[li], dims[li + 1]
        w, b = f32(rng.standard_normal((N, K)) / np.sqrt(K)), f32(rng.standard_normal(N) * 0.1)
        act = S.ACT_RELU if li in (0, 2) else S.ACT_NONE
        y = g.op("FULLY_CONNECTED", [t, g.const(w, f"fc{li}/w"), g.const(b, f"fc{li}/b")], [1, N], dict(fused_activation_function=act), name=f"fc{li}")
        layers.append(dict(name=f"fc{li}", out=y, a=t, w=w, b=b, act="relu" if act else "none", scale=None, res=None, HW=1, K=K, N=N))
        t = y
    return g.finish([x], [t]), dict(layers=layers, input=x, in_elems=100, logits=t)


def _conv(st, a, d=1, pad=S.PAD_SAME):
    return dict(padding=pad, stride_w=st, stride_h=st, dilation_w_factor=d, dilation_h_factor=d, fused_activation_function=a)


def mbconv_tail(H=9, W=8, Cl=16, C=24, Cr=4):
    """lead 1 x 1 (16 -> 24) -> dw 3 x 3 -> SE -> MUL -> projection 1 x 1 (24 -> 24, no activation) + lead's output -> 1 x 1 (24 -> 40,
    swish) -> MEAN -> FC.  The projection takes the squeeze-excite scale in its operand load and the residual in its epilogue; on a
    bf16 engine its A and its residual are stored as bf16."""
    rng = np.random.default_rng(22)
    g = GraphBuilder(description="mbconv tail")
    x = g.tensor([1, H, W, Cl], name="image")
    wl, bl = f32(rng.standard_normal((C, 1, 1, Cl)) / np.sqrt(Cl)), f32(rng.standard_normal(C) * 0.1)
    lead = g.op("CONV_2D", [x, g.const(wl, "lead/w"), g.const(bl, "lead/b")], [1, H, W, C], _conv(1, S.ACT_NONE), name="lead")
    wd, bd = f32(rng.standard_normal((1, 3, 3, C)) / 3.0), f32(rng.standard_normal(C) * 0.1)
    d = g.op("DEPTHWISE_CONV_2D", [lead, g.const(wd, "dw/w"), g.const(bd, "dw/b")], [1, H, W, C], dict(_conv(1, S.ACT_NONE), depth_multiplier=1), name="dw")
    d = g.op("MUL", [d, g.op("LOGISTIC", [d], [1, H, W, C])], [1, H, W, C], {}, name="dw/swish")
    m = g.op("MEAN", [d, g.const(i32([1, 2]))], [1, C], dict(keep_dims=0), name="se/mean")
    r = g.op("FULLY_CONNECTED", [m, g.const(f32(rng.standard_normal((Cr, C)) / np.sqrt(C)), "se/w1"), g.const(f32(rng.standard_normal(Cr) * 0.1 + 0.3), "se/b1")],
             [1, Cr], dict(fused_activation_function=S.ACT_RELU), name="se/fc1")
    e = g.op("FULLY_CONNECTED", [r, g.const(f32(rng.standard_normal((C, Cr)) / np.sqrt(Cr)), "se/w2"), g.const(f32(rng.standard_normal(C) * 0.1), "se/b2")],
             [1, C], dict(fused_activation_function=S.ACT_NONE), name="se/fc2")
    sg = g.op("LOGISTIC", [e], [1, C], name="se/scale")
    sr = g.op("RESHAPE", [sg, g.const(i32([1, 1, 1, C]))], [1, 1, 1, C], dict(new_shape=[1, 1, 1, C]))
    u = g.op("MUL", [d, sr], [1, H, W, C], {}, name="se/mul")
    wp, bp = f32(rng.standard_normal((C, 1, 1, C)) / np.sqrt(C)), f32(rng.standard_normal(C) * 0.1)
    p = g.op("CONV_2D", [u, g.const(wp, "proj/w"), g.const(bp, "proj/b")], [1, H, W, C], _conv(1, S.ACT_NONE), name="proj")
    a = g.op("ADD", [p, lead], [1, H, W, C], dict(fused_activation_function=S.ACT_NONE), name="block/add")
    Ct = 40
    wt, bt = f32(rng.standard_normal((Ct, 1, 1, C)) / np.sqrt(C)), f32(rng.standard_normal(Ct) * 0.1)
    top = g.op("CONV_2D", [a, g.const(wt, "top/w"), g.const(bt, "top/b")], [1, H, W, Ct], _conv(1, S.ACT_NONE), name="top")
    tops = g.op("MUL", [top, g.op("LOGISTIC", [top], [1, H, W, Ct])], [1, H, W, Ct], {}, name="top/swish")
    pm = g.op("MEAN", [tops, g.const(i32([1, 2]))], [1, Ct], dict(keep_dims=0), name="head/mean")
    wh = f32(rng.standard_normal((5, Ct)) / np.sqrt(Ct))
    y = g.op("FULLY_CONNECTED", [pm, g.const(wh, "head/w"), g.const(f32(np.zeros(5)), "head/b")], [1, 5], dict(fused_activation_function=S.ACT_NONE), name="head")
    HW = H * W
    layers = [dict(name="lead", out=lead, a=x, w=wl.reshape(C, Cl), b=bl, act="none", scale=None, res=None, HW=HW, K=Cl, N=C),
              dict(name="proj", out=a, a=d, w=wp.reshape(C, C), b=bp, act="none", scale=sg, res=lead, HW=HW, K=C, N=C),
              dict(name="top", out=tops, a=a, w=wt.reshape(Ct, C), b=bt, act="swish", scale=None, res=None, HW=HW, K=C, N=Ct),
              dict(name="head", out=y, a=pm, w=wh, b=np.zeros(5, np.float32), act="none", scale=None, res=None, HW=1, K=Ct, N=5)]
    return g.finish([x], [y]), dict(layers=layers, input=x, in_elems=H * W * Cl, logits=y)


def conv_stack(H=13, W=11, C=4):
    """3 x 3 (4 -> 20, ReLU6) -> 3 x 3 stride 2 (20 -> 12) -> 3 x 3 dilation 2 (12 -> 7, ReLU) -> MEAN -> FC: the implicit GEMM."""
    rng = np.random.default_rng(23)
    g = GraphBuilder(description="conv stack")
    x = t = g.tensor([1, H, W, C], name="image")
    convs = []
    for li, (co, s, d, act) in enumerate([(20, 1, 1, S.ACT_RELU6), (12, 2, 1, S.ACT_NONE), (7, 1, 2, S.ACT_RELU)]):
        w, b = f32(rng.standard_normal((co, 3, 3, C)) / np.sqrt(9 * C)), f32(rng.standard_normal(co) * 0.1)
        H, W = -(-H // s), -(-W // s)
        t = g.op("CONV_2D", [t, g.const(w, f"c{li}/w"), g.const(b, f"c{li}/b")], [1, H, W, co], _conv(s, act, d), name=f"c{li}")
        convs.append(dict(name=f"c{li}", out=t, elems=H * W * co))
        C = co
    m = g.op("MEAN", [t, g.const(i32([1, 2]))], [1, C], dict(keep_dims=0))
    y = g.op("FULLY_CONNECTED", [m, g.const(f32(rng.standard_normal((9, C)) / np.sqrt(C)), "head/w"), g.const(f32(np.zeros(9)), "head/b")], [1, 9],
             dict(fused_activation_function=S.ACT_NONE), name="head")
    return g.finish([x], [y]), dict(convs=convs, input=x, in_elems=13 * 11 * 4, logits=y)


GRAPHS = {"dense": dense_stack, "mbconv": mbconv_tail, "conv": conv_stack}


def _fetch(clf, step, n_per_clip):
    """A step's output as float64 [N_CLIPS, n]: fp32 storage, or bf16 storage in the first half of the value's block."""
    raw = clf.debug_fetch(-2 - step["out_v"], N_CLIPS, n_per_clip)
    if step["out_bf16"]:
        h = np.ascontiguousarray(raw).reshape(-1).view(np.uint16)[:N_CLIPS * n_per_clip]
        return (h.astype(np.uint32) << 16).view(np.float32).astype(np.float64).reshape(N_CLIPS, n_per_clip)
    return raw.astype(np.float64).reshape(N_CLIPS, n_per_clip)


def _step(steps, name):
    hit = [q for q in steps if q["name"] == name]
    assert len(hit) == 1, (name, [q["name"] for q in steps])
    return hit[0]


@pytest.mark.gpu
@pytest.mark.parametrize("graph,bx", [("dense", 0), ("dense", 2), ("mbconv", 0), ("mbconv", 2)])
def test_gemm_steps_reproduce_the_f64_layers(gpu, monkeypatch, graph, bx):
    for k in ("BNHIP_PW_FILL", "BNHIP_PW_NT", "BNHIP_PW_WM", "BNHIP_PW_LAT_TILES", "BNHIP_PW_B16", "BNHIP_PW_B16S", "BNHIP_PW_WS", "BNHIP_PW_TAIL", "BNHIP_PW_LAT"):
        monkeypatch.delenv(k, raising=False)
    blob, t = GRAPHS[graph]()
    x = np.random.default_rng(7).standard_normal((N_CLIPS, t["in_elems"])).astype(np.float32)
    keep64, keep32 = {}, {}
    Interpreter(blob, "f64").invoke(x, keep=keep64)
    Interpreter(blob).invoke(x, keep=keep32)
    clf = host.HipClassifier(blob, max_batch=4, lanes=1, autotune=False, bf16x3=bx, debug_no_reuse=True)
    try:
        d = clf.describe()
        steps = d["steps"]
        logits = clf.predict_batch(x.reshape(-1), N_CLIPS)
        assert d["precision"] == "f32" and not any(q["in_bf16"] or q["out_bf16"] for q in steps)      # an fp32 engine stores no bf16 value
        for L in t["layers"]:
            s = _step(steps, L["name"])
            # bf16x3 = 2: every GEMM with K >= 16, K % 4 == 0 on the split-bf16 family at its 128-row tile; 0: k_pw_gemm
            want_bx = 1 if bx == 2 and L["K"] >= 16 and L["K"] % 4 == 0 else 0
            assert s["kernel"] == "pw_gemm" and s["bx"] == want_bx and s["wm_full"] == (6 if want_bx else 0), (L["name"], s)
            assert s["fused_scale"] == (1 if L["scale"] is not None else 0) and s["fused_res"] == (1 if L["res"] is not None else 0), (L["name"], s)
            ref = np.asarray(keep64[L["out"]], np.float64).reshape(N_CLIPS, -1)
            r32 = np.asarray(keep32[L["out"]], np.float64).reshape(N_CLIPS, -1)
            got = logits.astype(np.float64).reshape(N_CLIPS, -1) if L["out"] == t["logits"] else _fetch(clf, s, ref.shape[1])
            scale = float(np.abs(ref).max())
            err, e32 = float(np.abs(got - ref).max()) / scale, float(np.abs(r32 - ref).max()) / scale
            gate = 4 * e32 + 2.0 ** -16
            print(f"{graph} bf16x3={bx} {L['name']}: err {err:.3e} (fp32 oracle {e32:.3e}, gate {gate:.3e})")
            assert np.isfinite(got).all() and err <= gate, (L["name"], err, e32)
    finally:
        clf.close()


@pytest.mark.gpu
def test_convolution_steps_reproduce_the_f64_layers(gpu):
    blob, t = conv_stack()
    x = np.random.default_rng(8).standard_normal((N_CLIPS, t["in_elems"])).astype(np.float32)
    keep64, keep32 = {}, {}
    Interpreter(blob, "f64").invoke(x, keep=keep64)
    Interpreter(blob).invoke(x, keep=keep32)
    clf = host.HipClassifier(blob, max_batch=4, lanes=1, autotune=False, debug_no_reuse=True)
    try:
        steps = clf.describe()["steps"]
        clf.predict_batch(x.reshape(-1), N_CLIPS)
        assert [q["kernel"] for q in steps].count("conv_igemm") == 3
        for L in t["convs"]:
            s = _step(steps, L["name"])
            assert s["kernel"] == "conv_igemm", s
            ref = np.asarray(keep64[L["out"]], np.float64).reshape(N_CLIPS, -1)
            r32 = np.asarray(keep32[L["out"]], np.float64).reshape(N_CLIPS, -1)
            got = _fetch(clf, s, L["elems"])
            scale = float(np.abs(ref).max())
            err, e32 = float(np.abs(got - ref).max()) / scale, float(np.abs(r32 - ref).max()) / scale
            gate = 4 * e32 + 2.0 ** -16
            print(f"conv {L['name']}: err {err:.3e} (fp32 oracle {e32:.3e}, gate {gate:.3e})")
            assert np.isfinite(got).all() and err <= gate, (L["name"], err, e32)
    finally:
        clf.close()


def _act64(v, act):
    return np.maximum(v, 0) if act == "relu" else v / (1 + np.exp(-v)) if act == "swish" else v


@pytest.mark.gpu
def test_one_product_engine_reproduces_fp64_on_the_operands_it_rounds(gpu, monkeypatch):
    """"precision": "bf16" with the residual stream and bf16 activation storage on (their defaults)."""
    for k in ("BNHIP_PW_FILL", "BNHIP_PW_NT", "BNHIP_PW_WM", "BNHIP_PW_B16", "BNHIP_PW_B16S", "BNHIP_PW_WS", "BNHIP_PW_TAIL", "BNHIP_BF16_ACT", "BNHIP_BF16_RESID"):
        monkeypatch.delenv(k, raising=False)
    blob, t = mbconv_tail()
    x = np.random.default_rng(9).standard_normal((N_CLIPS, t["in_elems"])).astype(np.float32)
    clf = host.HipClassifier(blob, max_batch=4, lanes=1, autotune=False, precision="bf16", debug_no_reuse=True)
    try:
        d = clf.describe()
        steps = d["steps"]
        logits = clf.predict_batch(x.reshape(-1), N_CLIPS)
        assert d["precision"] == "bf16"
        by = {L["name"]: L for L in t["layers"]}
        st = {n: _step(steps, n) for n in by}
        dw, se = [q for q in steps if q["kernel"] == "dwconv"], [q for q in steps if q["kernel"] == "se"]
        assert len(dw) == 1 and len(se) == 1, [q["kernel"] for q in steps]
        # storage: lead's output feeds the depthwise and the projection's residual (the bf16 residual stream), the depthwise output is the
        # projection's A (bf16 activation storage); the block output feeds `top` as bf16 A; what the pooling reads stays fp32
        assert st["lead"]["out_bf16"] == 1 and dw[0]["in_bf16"] == 1 and dw[0]["out_bf16"] == 1 and st["proj"]["in_bf16"] == 1
        assert st["proj"]["out_bf16"] == 1 and st["top"]["in_bf16"] == 1 and st["top"]["out_bf16"] == 0 and st["head"]["in_bf16"] == 0
        for n, s in st.items():
            assert s["kernel"] == "pw_gemm" and s["bx"] == (1 if by[n]["K"] >= 16 else 0) and s["wm_full"] == (6 if by[n]["K"] >= 16 else 0), s
        C = by["proj"]["K"]
        vals = {t["input"]: x.astype(np.float64).reshape(N_CLIPS, -1), by["lead"]["out"]: _fetch(clf, st["lead"], by["lead"]["HW"] * C),
                by["proj"]["a"]: _fetch(clf, dw[0], by["proj"]["HW"] * C), by["proj"]["scale"]: _fetch(clf, se[0], C),
                by["proj"]["out"]: _fetch(clf, st["proj"], by["proj"]["HW"] * C), by["top"]["out"]: _fetch(clf, st["top"], by["top"]["HW"] * by["top"]["N"]),
                by["head"]["out"]: logits.astype(np.float64).reshape(N_CLIPS, -1)}
        mean_step = [q for q in steps if q["kernel"] == "mean" and q["name"] == "head/mean"]
        assert len(mean_step) == 1
        vals[by["head"]["a"]] = _fetch(clf, mean_step[0], by["head"]["K"])
        for n in ("proj", "top", "head", "lead"):
            L, s = by[n], st[n]
            one = s["bx"] == 1                                         # (lead, K = 8, runs k_pw_gemm in fp32: no rounding)
            a = f32(vals[L["a"]].reshape(N_CLIPS, L["HW"], L["K"]))
            if L["scale"] is not None:
                a = a * f32(vals[L["scale"]]).reshape(N_CLIPS, 1, L["K"])          # the fp32 product every kernel forms
            w = L["w"]
            if one:
                a, w = bf16_round(a), bf16_round(w)
            acc64 = a.astype(np.float64) @ w.astype(np.float64).T + L["b"].astype(np.float64)
            acc32 = (a @ w.T + L["b"]).astype(np.float32)
            r64, r32 = _act64(acc64, L["act"]), _act64(acc32.astype(np.float32), L["act"]).astype(np.float32)
            if L["res"] is not None:
                res = vals[L["res"]].reshape(N_CLIPS, L["HW"], L["N"])
                r64, r32 = r64 + res, (r32 + f32(res)).astype(np.float32)
            got = vals[L["out"]].reshape(r64.shape)
            scale = float(np.abs(r64).max())
            e32 = float(np.abs(r32.astype(np.float64) - r64).max()) / scale
            allow = (4 * e32 + 2.0 ** -22) * scale
            ref = r64
            if s["out_bf16"]:                                          # the rounded reference, one bf16 ulp of the element on top
                ref = bf16_round(r64.astype(np.float32)).astype(np.float64)
                allow = allow + 2.0 ** (np.frexp(np.where(ref == 0, 2.0 ** -126, ref))[1] - 8)
            ratio = float((np.abs(got - ref) / allow).max())
            print(f"bf16 engine {n}: err {float(np.abs(got - ref).max()) / scale:.3e}, fp32 host {e32:.3e}, err / gate {ratio:.3f}, out_bf16 {s['out_bf16']}")
            assert np.isfinite(got).all() and ratio <= 1.0, (n, ratio)
    finally:
        clf.close()


@pytest.mark.parametrize("graph", ["dense", "mbconv", "conv"])
@pytest.mark.parametrize("kw", [dict(bf16x3=0), dict(bf16x3=2), dict(precision="bf16")], ids=["bf16x3=0", "bf16x3=2", "bf16"])
def test_plans_name_the_kernel_family_of_every_gemm_step(built_lib, graph, kw):
    """Without a device: which steps the three graphs plan, on which family (Step::bx) and planner tile."""
    blob, t = GRAPHS[graph]()
    plan = host.HipClassifier(blob, plan_only=True, max_batch=4, lanes=1, autotune=False, **kw)
    try:
        steps = plan.describe()["steps"]
    finally:
        plan.close()
    split = kw != dict(bf16x3=0)
    if graph == "conv":
        assert [q["kernel"] for q in steps].count("conv_igemm") == 3
        return
    for L in t["layers"]:
        s = _step(steps, L["name"])
        want_bx = 1 if split and L["K"] >= 16 and L["K"] % 4 == 0 else 0
        assert s["kernel"] == "pw_gemm" and s["bx"] == want_bx and s["wm_full"] == (6 if want_bx else 0), (L["name"], s)
        assert s["fused_scale"] == (1 if L["scale"] is not None else 0) and s["fused_res"] == (1 if L["res"] is not None else 0), (L["name"], s)


@pytest.mark.parametrize("model", ["tiny", "v24", "perch"])
def test_no_plan_hands_a_six_product_gemm_bf16_activations(built_lib, monkeypatch, model):
    """PwParams::a_bf16 with prec = 0 is a combination no kernel but k_pw_bx3 / k_pw_bx3p reads correctly (the six-product k_pw_b16 has no
    bf16-A form; pw_b16_ok refuses it, pw_lat_ok and pw_ws_ok always did).  The planner cannot produce it: bf16 storage is marked by
    Engine::mark_bf16_storage, which returns at once unless the engine's precision is bf16 - and then every GEMM runs one product.
    Checked here on the plans (a plan-only engine marks nothing; the created engines of the tests above assert the same on a device):
    no fp32 engine, whatever bf16x3 and BNHIP_PW_B16 say, has a step that reads or writes a bf16 value."""
    from birdnet_go_amd import synth_model as sm
    cfg = {"tiny": sm.tiny_config, "v24": sm.SynthConfig, "perch": sm.perch_config}[model]()
    blob = sm.build_model(cfg)
    for b16 in (None, "0", "2"):
        if b16 is None:
            monkeypatch.delenv("BNHIP_PW_B16", raising=False)
        else:
            monkeypatch.setenv("BNHIP_PW_B16", b16)
        for kw in (dict(bf16x3=0), dict(bf16x3=1), dict(bf16x3=2), dict(precision="bf16"), dict(precision="bf16", bf16x3=0)):
            plan = host.HipClassifier(blob, plan_only=True, **kw)
            try:
                d = plan.describe()
            finally:
                plan.close()
            gemms = [q for q in d["steps"] if q["kernel"] == "pw_gemm"]
            assert len(gemms) >= 3
            if d["precision"] != "bf16":
                assert not any(q["in_bf16"] or q["out_bf16"] for q in d["steps"]), (model, kw, b16)
            else:
                assert all(q["bx"] == 1 for q in gemms if q["in_bf16"]), (model, kw, b16)     # bf16 A only into the split-bf16 family, at one product
