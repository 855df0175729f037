"""Kernel-level exactness of the pointwise / dense GEMM family (csrc/pw_gemm.hip, pw_bx3.hip, pw_b16.hip, pw_ws.hip), without a model:
tools/ubench/pw64_lab drives launch_pw_gemm, launch_pw_bx3 and launch_conv_igemm over a fixed case list and holds every output element
to a plain fp64 loop nest act(sum_k a scale w + bias) + res (gates: the lab's comments and DESIGN.md, "Pointwise GEMM family: what is
pinned per kernel form").  tests/test_pw_lab.py compares the forms with each other bit for bit, which cannot see an error in what they
share (the epilogue, the weight image, the split); the model-level tests see them through logits and, for calls of a few clips, only
at the tile pw_fill_grid shrank them to.

Here: the coverage conditions on the case list and the lab's own fp64 reference against the oracle run without a GPU; on the device the
list runs in two processes (BNHIP_PW_FILL is read once per process) - with BNHIP_PW_FILL=0 every dispatcher branch at the tile it
names, without it the cases whose tile pw_fill_grid (or launch_conv_igemm's small-grid rule) changes."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_SWITCHES = ("BNHIP_PW_FILL", "BNHIP_PW_NT", "BNHIP_PW_WM", "BNHIP_PW_LAT_TILES")
ACTS = {"none", "relu", "relu6", "swish", "sigmoid", "hardswish"}          # every activation apply_act implements


@pytest.fixture(scope="module")
def lab(built_lib, tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("pw64_lab") / "pw64_lab")
    libdir = os.path.dirname(built_lib)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "birdnet-go_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "ubench", "pw64_lab.cpp"), "-L", libdir, "-lbnhip", "-Wl,-rpath," + libdir],
                   check=True, capture_output=True, timeout=600)
    return exe


def _env(fill0):
    env = {k: v for k, v in os.environ.items() if k not in ENV_SWITCHES}
    if fill0:
        env["BNHIP_PW_FILL"] = "0"
    return env


def parse(out):
    m = re.search(r"^SUMMARY (\{.*\})$", out, re.M)
    assert m, out[-2000:]
    return json.loads(m.group(1))


def cases_of(listing):
    rows = [dict(kv.split("=", 1) for kv in ln.split()[2:]) | {"name": ln.split()[1]} for ln in listing.splitlines() if ln.startswith("CASE ")]
    return [{k: (int(v) if re.fullmatch(r"-?\d+", v) else v) for k, v in r.items()} for r in rows]


def _listing(lab, fill0):
    r = subprocess.run([lab, "--list"], capture_output=True, text=True, timeout=600, env=_env(fill0))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert parse(r.stdout)["cases"] == len(re.findall(r"^CASE ", r.stdout, re.M)) and "FAIL" not in r.stdout
    assert f"PASS {1 if fill0 else 2}" in r.stdout
    return r.stdout


@pytest.fixture(scope="module")
def listing(lab):
    return _listing(lab, True)


@pytest.fixture(scope="module")
def listing2(lab):
    return _listing(lab, False)


def _pw(listing, form=None):
    return [c for c in cases_of(listing) if c["kind"] == "pw" and (form is None or c["form"] == form)]


TILED = ["k_pw_gemm", "k_pw_pipe", "k_pw_bx3", "k_pw_bx3p", "k_pw_b16_six", "k_pw_b16_one", "k_pw_bx3_one", "k_pw_bx3p_one"]
ALL_FORMS = TILED + ["k_pw_naive", "k_pw_b16s", "k_pw_ws_six", "k_pw_ws_one", "k_pw_lat", "k_pw_gemm_IM"]


def test_first_pass_runs_every_dispatcher_branch_at_the_tile_it_names(listing):
    cs = cases_of(listing)
    assert len({c["name"] for c in cs}) == len(cs) >= 400
    assert {c["form"] for c in cs} == set(ALL_FORMS)
    for c in cs:                                                           # the predicted tile is the requested one
        assert (c["run_rows"], c["run_nt"]) == (c["req_rows"], c["req_nt"]) or not c["tiled"], c["name"]
        assert c["M"] * c["N"] * c["K"] <= 70e6, c["name"]                  # (multiply-adds on the host per case)
    nts = lambda form, **kw: {c["run_nt"] for c in _pw(listing, form) if all(c[k] == v for k, v in kw.items())}
    full = set(range(1, 9))
    assert nts("k_pw_gemm", wm=1, run_rows=64) == full and nts("k_pw_gemm", wm=2, run_rows=128) == full
    assert nts("k_pw_pipe", wm=3, run_rows=64) == {1, 2, 3, 4} == nts("k_pw_pipe", wm=4, run_rows=128)
    assert nts("k_pw_bx3", wm=5, run_rows=64) == full and nts("k_pw_bx3", wm=6, run_rows=128) == full
    # k_pw_bx3p wherever pw_bx3p_ok holds (two operand buffers within 80 KB, more than one slab): the rule restated
    fits = lambda nt, wm: 2 * (64 * wm * 40 + 12 * nt * 16 * 4) * 4 <= 80 * 1024
    for c in _pw(listing):
        if c["wm"] in (7, 8):
            want = fits(c["nt"], c["wm"] - 6) and c["K"] > 32
            assert c["form"] in (("k_pw_bx3p", "k_pw_bx3p_one") if want else ("k_pw_bx3", "k_pw_bx3_one")), c["name"]
    assert nts("k_pw_bx3p", wm=7) == full and nts("k_pw_bx3p", wm=8) == {1, 2, 3, 4, 5, 6}
    assert nts("k_pw_b16_six", wm=10, run_rows=64) == full and nts("k_pw_b16_six", wm=9, run_rows=128) == full
    assert nts("k_pw_b16_one", a16=0, run_rows=128) == full == nts("k_pw_b16_one", a16=1, run_rows=128)
    assert all(c["run_rows"] == 128 and c["prec"] == 1 for c in _pw(listing, "k_pw_b16_one"))
    # the 64-row fall-through of a one-product engine
    assert nts("k_pw_bx3_one", wm=10, run_rows=64) == full and nts("k_pw_bx3_one", wm=5, a16=1) == full
    assert {c["a16"] for c in _pw(listing, "k_pw_bx3p_one")} == {0, 1}
    # with every full-tile case a shape of at least two row blocks and two column blocks, per form and nt, full and ragged last blocks
    for form in TILED[:7]:
        for nt in {c["run_nt"] for c in _pw(listing, form)}:
            two = [c for c in _pw(listing, form) if c["run_nt"] == nt and c["mblk"] >= 2 and c["nblk_n"] >= 2]
            assert any(c["N"] % (16 * nt) == 0 and c["M"] % c["run_rows"] == 0 for c in two), (form, nt)
            assert any(c["N"] % (16 * nt) and c["M"] % c["run_rows"] for c in two), (form, nt)
    # k_pw_b16s: NT 1 / 2 x NS 1 .. 6 x scale x A storage; N = 32 and 28
    s = _pw(listing, "k_pw_b16s")
    assert {(c["run_nt"], c["slabs"], c["scale"], c["a16"]) for c in s} == {(a, b, c, d) for a in (1, 2) for b in range(1, 7) for c in (0, 1) for d in (0, 1)}
    assert {12, 16, 28, 32} <= {c["N"] for c in s} and all(c["wm"] == 11 and c["prec"] == 1 for c in s)
    # k_pw_ws
    ws = _pw(listing, "k_pw_ws_six")
    assert {(c["slabs"], c["run_nt"]) for c in ws} == {(a, b) for a in (3, 4, 5, 6) for b in (4, 6, 8)} | {(8, 4), (8, 6), (10, 4)}
    assert any(c["M"] == 16 * 16 for c in ws) and any(((c["M"] + 15) // 16) % 2 and c["M"] % 16 for c in ws)      # M / 16 = 2 WS_NW exactly; a ragged last tile pair
    w1 = _pw(listing, "k_pw_ws_one")
    assert {(c["slabs"], c["a16"]) for c in w1} == {(a, b) for a in (3, 4, 5, 6) for b in (0, 1)} and all(c["K"] % 8 == 0 for c in w1 if c["a16"])
    assert all(c["sw"] & 32 and c["wm"] == 12 and not c["scale"] for c in ws + w1)
    # k_pw_lat and k_pw_naive
    lat = _pw(listing, "k_pw_lat")
    assert {(c["run_nt"], c["scale"]) for c in lat} == {(1, 0), (1, 1), (2, 0), (2, 1)} and {256, 260, 416, 512} == {c["K"] for c in lat}
    assert all(c["K"] == 256 and ((c["M"] + 15) // 16) * ((c["N"] + 15) // 16) >= 1024 for c in lat if c["run_nt"] == 2)
    assert all(not c["sw"] & 64 for c in lat) and all(c["sw"] & 64 for c in _pw(listing) if c["form"] not in ("k_pw_lat", "k_pw_gemm", "k_pw_pipe", "k_pw_naive"))
    assert {5, 18} == {c["K"] for c in _pw(listing, "k_pw_naive")}
    # the contract hole: six products on bf16 A asked onto k_pw_b16 stays on k_pw_bx3
    hole = [c for c in _pw(listing) if c["prec"] == 0 and c["a16"]]
    assert any(c["wm"] == 9 for c in hole) and any(c["wm"] == 10 for c in hole) and any(c["sw"] & 2 for c in hole)
    assert all(c["form"] in ("k_pw_bx3", "k_pw_bx3p") and c["K"] % 8 == 0 for c in hole)


def test_first_pass_covers_rows_columns_k_scale_and_epilogue(listing):
    pw = _pw(listing)
    main = ["k_pw_gemm", "k_pw_bx3", "k_pw_b16_six", "k_pw_b16_one"]
    for form in main:
        f = _pw(listing, form)
        assert {1, 15, 16, 17, 63, 64, 65, 127, 129} <= {c["M"] for c in f}, form
        assert any(c["M"] >= 2 * 128 + 1 and c["M"] % 128 for c in f), form
        assert {4, 12, 16, 20, 36, 68, 132, 7, 33, 130} <= {c["N"] for c in f}, form
        assert {16, 20, 32, 36, 64, 96, 100, 128, 136, 232} <= {c["K"] for c in f if not c["a16"]}, form
        # the scale: a 16-row tile inside one clip (the LDS path of k_pw_b16), over two or three clips, a block inside one clip
        assert {1, 16, 48, 7, 23} <= {c["HW"] for c in f if c["scale"]} and any(c["HW"] > 128 for c in f if c["scale"]), form
    assert {1, 16, 48, 7, 23} <= {c["HW"] for c in _pw(listing, "k_pw_lat") if c["scale"]} and any(c["HW"] > 128 for c in _pw(listing, "k_pw_lat"))
    assert all(not (c["o16"] or c["r16"]) for c in pw if c["N"] % 4)         # N % 4 != 0: fp32 storage only
    assert all(c["K"] % 8 == 0 for c in pw if c["a16"])
    for form in ("k_pw_pipe", "k_pw_bx3p"):                                  # prologue / steady / drain
        sl = {c["slabs"] for c in _pw(listing, form)}
        assert {2, 3} <= sl and any(v >= 4 for v in sl), (form, sl)
    assert 1 in {c["slabs"] for c in _pw(listing, "k_pw_gemm") if c["wm"] in (3, 4)}      # (one slab: the pipelined request of K = 32 is legal, K = 16 / 20 falls to the plain kernel)
    assert any(c["slabs"] == 1 and c["K"] == 32 for c in _pw(listing, "k_pw_pipe"))
    # epilogue
    for form in ("k_pw_gemm", "k_pw_pipe", "k_pw_bx3", "k_pw_bx3p", "k_pw_b16_six", "k_pw_b16_one", "k_pw_bx3_one", "k_pw_ws_six", "k_pw_ws_one", "k_pw_lat", "k_pw_b16s"):
        f = _pw(listing, form)
        assert {(c["r16"], c["o16"]) for c in f if c["res"]} == {(0, 0), (1, 0), (0, 1), (1, 1)}, form
        assert {c["bias"] for c in f} == {0, 1} and any(c["o16"] and not c["res"] for c in f), form
        assert {c["act"] for c in f} == ACTS, form
    shares = [float(c["clip"]) for c in cases_of(listing) if c["act"] == "relu6"]
    assert len(shares) >= 20 and min(shares) >= 0.01 and max(shares) <= 0.50, (min(shares), max(shares))


def test_first_pass_covers_the_implicit_gemm(listing):
    ig = [c for c in cases_of(listing) if c["kind"] == "ig"]
    assert {(3, 3), (5, 5), (2, 2), (1, 1)} == {(c["kh"], c["kw"]) for c in ig} and any(c["kh"] == 1 and c["stride"] == 2 for c in ig)
    assert any(c["dil"] == 2 for c in ig) and {0, 1, 2} <= {c["pt"] for c in ig} and {0, 1, 2} <= {c["pl"] for c in ig}
    assert {(1, 0), (1, 1), (2, 0), (2, 1)} <= {(c["stride"], c["H"] % 2) for c in ig}
    assert {4, 8, 12} <= {c["Cin"] for c in ig} and {7, 20, 48} == {c["N"] for c in ig} and {0, 1} == {c["valid"] for c in ig}
    assert all(c["Cin"] % 4 == 0 and c["K"] >= 32 and c["form"] == "k_pw_gemm_IM" for c in ig)
    big = [c for c in ig if c["mblk"] * c["nblk_n"] >= 64]
    assert len(big) >= 3 and {(128, 2), (128, 4)} <= {(c["run_rows"], c["run_nt"]) for c in big} and any(c["run_rows"] == 64 for c in big)
    assert all((c["run_rows"], c["run_nt"]) == (64, 1) for c in ig if c not in big)
    assert {c["act"] for c in ig} == ACTS and {c["bias"] for c in ig} == {0, 1}


def test_second_pass_is_the_shrink(listing2):
    cs = cases_of(listing2)
    assert 20 <= len(cs) <= 60
    for c in cs:                                                           # every predicted tile differs from the requested one
        assert c["tiled"] and (c["run_rows"], c["run_nt"]) != (c["req_rows"], c["req_nt"]), c["name"]
    pw = [c for c in cs if c["kind"] == "pw"]
    half = lambda n, k: n if k == 0 else half((n + 1) // 2, k - 1)
    assert any(c["req_rows"] == 128 and c["run_rows"] == 64 and c["run_nt"] == c["req_nt"] for c in pw)          # 128 -> 64 rows only
    assert any(c["req_rows"] == 64 and c["run_nt"] == half(c["req_nt"], 1) != c["req_nt"] for c in pw)           # nt halved once
    assert any(c["run_nt"] == half(c["req_nt"], 2) != half(c["req_nt"], 1) for c in pw)                        # ... twice
    assert any(c["req_nt"] in (3, 5) for c in pw)                                                              # (odd widths round up)
    assert any(c["wm"] in (3, 4) and c["form"] == "k_pw_gemm" for c in pw) and any(c["wm"] in (7, 8) and c["form"] == "k_pw_bx3" for c in pw)
    assert any(c["wm"] == 9 and c["prec"] == 1 and c["form"] == "k_pw_bx3_one" and c["a16"] == a for c in pw for a in (0, 1))
    assert not any(c["form"] in ("k_pw_pipe", "k_pw_bx3p", "k_pw_b16_one") for c in pw)
    assert {"k_pw_gemm", "k_pw_bx3", "k_pw_b16_six", "k_pw_bx3_one", "k_pw_gemm_IM"} == {c["form"] for c in cs}
    assert any(c["M"] <= 48 for c in pw)                                                                        # one clip of a late layer
    ig = [c for c in cs if c["kind"] == "ig"]
    assert len(ig) >= 5 and all((c["run_rows"], c["run_nt"]) == (64, 1) for c in ig)                            # launch_conv_igemm's small-grid rule


def _ref_cases(listing, listing2):
    """About ten cases by property rather than by name: the first of each kind in list order."""
    cs, pick = cases_of(listing), []
    first = lambda pred: next(c["name"] for c in cs if pred(c))
    pick.append(first(lambda c: c["form"] == "k_pw_gemm" and not c["scale"] and c["res"]))
    pick.append(first(lambda c: c["form"] == "k_pw_bx3" and c["scale"] and c["HW"] == 48 and c["M"] % 48 == 0))
    pick.append(first(lambda c: c["form"] == "k_pw_b16_six" and c["scale"] and c["HW"] == 7 and c["res"]))
    pick.append(first(lambda c: c["form"] == "k_pw_b16_one" and c["scale"] and c["HW"] == 16 and not c["a16"]))
    pick.append(first(lambda c: c["form"] == "k_pw_b16_one" and c["a16"] and not c["scale"] and c["K"] % 32))
    pick.append(first(lambda c: c["form"] == "k_pw_b16s" and c["scale"] and c["act"] == "swish"))
    pick.append(first(lambda c: c["form"] == "k_pw_ws_six" and c["K"] % 32 and c["res"]))
    pick.append(first(lambda c: c["form"] == "k_pw_lat" and c["scale"] and c["K"] == 260))
    pick.append(first(lambda c: c["form"] == "k_pw_naive" and c["scale"]))
    pick.append(first(lambda c: c["kind"] == "ig" and c["dil"] == 2 and not c["valid"]))
    pick.append(first(lambda c: c["kind"] == "ig" and c["stride"] == 2 and c["kh"] == 5 and c["act"] == "hardswish"))
    pick.append(first(lambda c: c["kind"] == "ig" and c["kh"] == 2 and c["valid"]))
    pick.append(next(c["name"] for c in cases_of(listing2) if c["form"] == "k_pw_bx3_one" and c["scale"]))
    assert len(set(pick)) == len(pick)
    return pick


def _oracle(tmp_path, meta, mi):
    """The dumped case as TFLite graphs through the fp64 oracle -> [M, N]."""
    from birdnet_go_amd import tflite_schema as S
    from birdnet_go_amd.tflite_build import GraphBuilder
    from oracle.interp import Interpreter
    f32 = lambda fn: np.fromfile(tmp_path / fn, np.float32)
    M, N, K, HW = (mi[q] for q in ("M", "N", "K", "HW"))
    one = mi["one"]
    w = f32("wr.f32" if one else "w.f32")
    bias = f32("b.f32")
    fused = {"relu": S.ACT_RELU, "relu6": S.ACT_RELU6}.get(meta["act"], S.ACT_NONE)

    def act(g, t, shape):
        if meta["act"] == "swish":
            return g.op("MUL", [t, g.op("LOGISTIC", [t], shape)], shape, {})
        if meta["act"] == "sigmoid":
            return g.op("LOGISTIC", [t], shape)
        if meta["act"] == "hardswish":
            return g.op("HARD_SWISH", [t], shape)
        return t

    def run(g, x, y, xin, batch):
        keep = {}
        Interpreter(g.finish([x], [y]), "f64").invoke(xin.reshape(batch, -1), keep=keep)
        out = np.asarray(keep[y])
        assert out.dtype == np.float64
        return out.reshape(-1, N)
    res = f32("res.f32").astype(np.float64).reshape(M, N) if mi["res"] else 0.0
    if meta["kind"] == "ig":
        B, H, W, Cin, Ho, Wo = (mi[q] for q in ("B", "H", "W", "Cin", "Ho", "Wo"))
        g = GraphBuilder(description="pw64 lab case")
        x = g.tensor([1, H, W, Cin], name="image")
        y = g.op("CONV_2D", [x, g.const(w.reshape(N, mi["kh"], mi["kw"], Cin)), g.const(bias)], [1, Ho, Wo, N],
                 dict(padding=S.PAD_VALID if mi["valid"] else S.PAD_SAME, stride_w=mi["stride"], stride_h=mi["stride"], dilation_w_factor=mi["dil"],
                      dilation_h_factor=mi["dil"], fused_activation_function=fused))
        return run(g, x, act(g, y, [1, Ho, Wo, N]), f32("a.f32"), B)
    # one-product cases: the rounded operands the dump contains (a scale already applied and rounded), so no MUL
    a = f32("xr.f32" if one else "a.f32").reshape(M, K)
    if not HW or one:
        g = GraphBuilder(description="pw64 lab case")                     # FULLY_CONNECTED, every row a batch entry
        x = g.tensor([1, K], name="rows")
        y = g.op("FULLY_CONNECTED", [x, g.const(w.reshape(N, K)), g.const(bias)], [1, N], dict(fused_activation_function=fused))
        return run(g, x, act(g, y, [1, N]), a, M) + res
    # scaled: a 1 x 1 CONV_2D behind a MUL with the clip's scale row (a constant: one graph per clip), the residual as an ADD
    scale = f32("scale.f32").reshape(-1, K)
    out = np.zeros((M, N))
    for b in range(scale.shape[0]):
        rows = slice(b * HW, min((b + 1) * HW, M))
        n = rows.stop - rows.start
        g = GraphBuilder(description="pw64 lab case")
        x = g.tensor([1, n, 1, K], name="image")
        u = g.op("MUL", [x, g.const(scale[b].reshape(1, 1, 1, K))], [1, n, 1, K], {})
        y = g.op("CONV_2D", [u, g.const(w.reshape(N, 1, 1, K)), g.const(bias)], [1, n, 1, N],
                 dict(padding=S.PAD_SAME, stride_w=1, stride_h=1, dilation_w_factor=1, dilation_h_factor=1, fused_activation_function=fused))
        y = act(g, y, [1, n, 1, N])
        if mi["res"]:
            y = g.op("ADD", [y, g.const(f32("res.f32").reshape(M, N)[rows].reshape(1, n, 1, N))], [1, n, 1, N], dict(fused_activation_function=S.ACT_NONE))
        out[rows] = run(g, x, y, a[rows], 1)
    return out


def test_lab_reference_agrees_with_the_f64_oracle(lab, listing, listing2, tmp_path):
    """The lab's fp64 loop nest against the project's independent oracle on the same data: two fp64 evaluations that differ in summation
    order only (at most 1152 terms of magnitude <= scale: ~1152 * 2^-53 ~ 1.3e-13) -> 1e-12 of the output scale.  One-product cases are
    fed the rounded operands the dump contains."""
    names = _ref_cases(listing, listing2)
    assert len(names) >= 10
    kinds = set()
    for i, name in enumerate(names):
        d = tmp_path / str(i)
        d.mkdir()
        r = subprocess.run([lab, "--ref-dump", name, str(d)], capture_output=True, text=True, timeout=600, env=_env(True))
        assert r.returncode == 0, r.stdout[-2000:]
        meta = dict(ln.strip().split("=") for ln in open(d / "meta.txt"))
        mi = {k: int(v) for k, v in meta.items() if re.fullmatch(r"-?\d+", v)}
        ref = _oracle(d, meta, mi)
        got = np.fromfile(d / "y.f64", np.float64).reshape(ref.shape)
        scale = float(np.abs(ref).max())
        err = float(np.abs(got - ref).max()) / scale
        print(f"{name}: lab fp64 reference vs oracle f64: {err:.3e} of the output scale {scale:.3g}")
        assert scale > 0 and err <= 1e-12, (name, err)
        kinds.add((meta["kind"], mi["one"], bool(mi["HW"]), bool(mi["res"])))
    assert {k[0] for k in kinds} == {"pw", "ig"} and {k[1] for k in kinds} == {0, 1} and {k[2] for k in kinds} == {False, True}


def _run(lab, fill0):
    """One pass in one process with its own time limit (a pass is a few seconds: the host references dominate)."""
    return subprocess.run([lab], capture_output=True, text=True, timeout=300, env=_env(fill0))


def _check(r, listing, npass):
    tail = "\n".join(r.stdout.splitlines()[-40:]) + r.stderr[-2000:]
    got = parse(r.stdout)
    fails = [ln for ln in r.stdout.splitlines() if ln.startswith("FAIL")]
    print("\n".join(ln for ln in r.stdout.splitlines() if ln.startswith("FORM ")))
    assert f"PASS {npass}" in r.stdout and got["pass"] == npass, tail
    assert got["failures"] == 0 and not fails, "\n".join(fails[:40])
    assert r.returncode == 0, tail
    want = cases_of(listing)
    assert got["ran"] == got["cases"] == len(want), (got, len(want))
    counts = {m.group(1): int(m.group(2)) for m in re.finditer(r"^FORM (\S+) \| cases=(\d+)", r.stdout, re.M)}
    for form in {c["form"] for c in want}:                                 # every form named in the list really ran
        assert counts.get(form, 0) == sum(c["form"] == form for c in want) > 0, (form, counts)


@pytest.mark.gpu
def test_every_kernel_form_matches_fp64_on_the_device(gpu, lab, listing, listing2):
    """Two processes, no retry; the second is not started after a first one that ended by a HIP error, a signal or its time limit
    (subprocess.run raises on the latter)."""
    r1 = _run(lab, True)
    assert r1.returncode in (0, 1), "\n".join(r1.stdout.splitlines()[-40:]) + r1.stderr[-2000:]
    r2 = _run(lab, False)
    _check(r1, listing, 1)
    assert r2.returncode in (0, 1), "\n".join(r2.stdout.splitlines()[-40:]) + r2.stderr[-2000:]
    _check(r2, listing2, 2)
