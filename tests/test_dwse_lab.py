"""Kernel-level exactness of the plain depthwise, pooling and squeeze-excite kernels (csrc/dwconv.hip), without a model:
tools/ubench/dwse_lab drives launch_dwconv, launch_mean_partial / launch_mean_finish and launch_se over a fixed case list and holds
every output element, every slab sum in the kernel's own slab order and the totals per (clip, channel) to a plain fp64 loop nest
(gates: the lab's comments and DESIGN.md, "Plain depthwise, pooling and squeeze-excite: what is pinned per kernel").  The model-level
tests see these kernels only through logits, only at the shipped shapes, and k_dwconv_t only where the tuner preferred it that day.

Here: the coverage condition on the case list and the lab's own fp64 reference against the oracle run without a GPU; on the device
the list runs once per process - the default one, and one with BNHIP_DW_PREFETCH=0 (the switch is read once per process) for the
row-by-row load form of bf16 inputs."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lab(built_lib, tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("dwse_lab") / "dwse_lab")
    libdir = os.path.dirname(built_lib)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "birdnet-go_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "ubench", "dwse_lab.cpp"), "-L", libdir, "-lbnhip", "-Wl,-rpath," + libdir],
                   check=True, capture_output=True, timeout=600)
    return exe


def parse(out):
    m = re.search(r"^SUMMARY (\{.*\})$", out, re.M)
    assert m, out[-2000:]
    return json.loads(m.group(1))


def cases_of(listing, kind):
    rows = [dict(kv.split("=", 1) for kv in ln.split()[2:]) | {"name": ln.split()[1]} for ln in listing.splitlines() if ln.startswith("CASE ")]
    out = []
    for r in rows:
        if r["kind"] == kind:
            out.append({k: (int(v) if re.fullmatch(r"-?\d+", v) else v) for k, v in r.items()})
    return out


@pytest.fixture(scope="module")
def listing(lab):
    r = subprocess.run([lab, "--list"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_case_list_covers_the_tiled_depthwise(listing):
    t = cases_of(listing, "dwt")
    assert parse(listing)["cases"] == len(re.findall(r"^CASE ", listing, re.M)) and "FAIL" not in listing
    # the four (K, S) forms, each with the four storages; the bf16-input ones are what the second process runs
    for k, s in ((3, 1), (3, 2), (5, 1), (5, 2)):
        have = {(c["in16"], c["out16"]) for c in t if (c["kh"], c["sh"]) == (k, s)}
        assert have == {(0, 0), (1, 0), (0, 1), (1, 1)}, (k, s, have)
        assert all(c["form"] == f"k_dwconv_t<{k},{s}>" and c["kh"] == c["kw"] and c["sh"] == c["sw"] for c in t if (c["kh"], c["sh"]) == (k, s))
    assert {c["act"] for c in t} == {"none", "relu6", "swish"}
    assert {c["bias"] for c in t} == {0, 1} and {c["part"] for c in t} == {0, 1}
    assert any(c["in16"] and not c["part"] for c in t) and any(c["out16"] and not c["bias"] for c in t)
    # geometry: ragged last tile row and column, images smaller than a tile, a kernel larger than the image
    assert any(c["Ho"] % c["TH"] and c["Wo"] % c["TW"] for c in t)
    assert any((c["H"], c["W"]) == (1, 1) for c in t) and any((c["H"], c["W"]) == (1, 3) for c in t)
    assert any(c["H"] == 2 and c["kh"] == 5 for c in t)
    # stride 2: odd sizes, and even sizes, where SAME pads bottom and right only (3 x 3: nothing in front)
    assert any(c["sh"] == 2 and c["H"] % 2 and c["W"] % 2 and not c["valid"] for c in t)
    assert any(c["sh"] == 2 and c["kh"] == 3 and c["H"] % 2 == 0 and c["W"] % 2 == 0 and not c["valid"] and (c["pt"], c["pl"]) == (0, 0) for c in t)
    assert any(c["sh"] == 2 and c["kh"] == 5 and c["H"] % 2 == 0 and c["W"] % 2 == 0 and not c["valid"] and (c["pt"], c["pl"]) == (1, 1) for c in t)
    assert {(c["kh"], c["sh"]) for c in t if c["valid"] and (c["pt"], c["pl"]) == (0, 0)} == {(3, 1), (3, 2), (5, 1), (5, 2)}
    # block geometry
    assert {4, 12, 20, 64, 256, 260} <= {c["C"] for c in t}
    for c in t:
        assert c["CX"] == min(c["C"] // 4, 64) and c["block"] == max(64, c["CX"] * c["PY"]) and c["nblk"] == c["B"] * c["tchunks"] * c["cchunks"]
        assert c["H"] <= 40 and c["W"] <= 40 and c["B"] <= 3
    assert any(c["C"] == 12 and c["block"] == 255 for c in t)                              # blocks of 255 threads
    assert any(c["block"] == 64 and c["live_last"] == 2 for c in t)                      # floored to 64 threads, 2 live
    assert any(c["C"] == 260 and c["cchunks"] == 2 and c["tchunks"] > 1 for c in t)        # a second channel chunk with one live quad
    assert any(c["tiles"] < 256 // c["CX"] for c in t)                                   # fewer tiles than PY
    assert any(c["tiles"] > 3 * c["PY"] and c["tiles"] % c["PY"] for c in t)               # more than 3 PY, ragged last chunk
    assert {1, 5, 8, 13} <= {c["nblk"] for c in t} and any(c["nblk"] > 8 and c["nblk"] % 8 for c in t)
    assert {c["B"] for c in t} == {1, 3}


def test_case_list_covers_the_generic_depthwise_the_means_and_squeeze_excite(listing):
    g = cases_of(listing, "dwg")
    assert {(3, 1), (1, 5), (2, 2), (7, 7)} <= {(c["kh"], c["kw"]) for c in g}
    assert {(1, 2), (2, 1), (3, 3)} <= {(c["sh"], c["sw"]) for c in g}
    assert {1, 6, 8} <= {c["C"] for c in g}
    assert {"none", "relu", "relu6", "swish", "sigmoid", "hardswish"} == {c["act"] for c in g}          # every activation of apply_act
    assert any(not c["bias"] for c in g)
    assert {c["form"] for c in g} == {"k_dwconv<4>", "k_dwconv<1>"}
    assert all((c["form"] == "k_dwconv<4>") == (c["C"] % 4 == 0) and not c["in16"] and not c["out16"] for c in g)
    assert any(c["B"] * c["Ho"] * c["Wo"] * c["C"] > 256 and (c["B"] * c["Ho"] * c["Wo"] * c["C"]) % 256 for c in g if c["form"] == "k_dwconv<1>")

    m = cases_of(listing, "mean")
    assert {1, 511, 512, 513, 1500} == {c["HW"] for c in m} and {1, 3, 63, 64, 65, 130} == {c["C"] for c in m} and {1, 3} == {c["B"] for c in m}

    se = cases_of(listing, "se")
    full = [c for c in se if not c["probe"]]
    assert {0, 64, 256, 1024} == {c["threads"] for c in full}
    assert {4, 6, 24, 96, 1152, 2048, 4096, 4098, 4100} == {c["C"] for c in full}
    assert {1, 3, 4, 17, 48} == {c["Cr"] for c in full} and {1, 2, 3, 96, 130} == {c["S"] for c in full}
    assert {"relu", "swish"} == {c["act1"] for c in full} and {"sigmoid", "none"} == {c["act2"] for c in full}
    assert {0, 1} == {c["b1"] for c in full} == {c["b2"] for c in full}
    live = [float(c["relu_live"]) for c in full if c["act1"] == "relu"]                    # no ReLU case whose FC1 outputs are all stopped
    assert len(live) >= 3 and min(live) > 0 and any(v < 1 for v in live), live
    # the named paths
    assert any(c["P"] == 1 and c["S"] > 1 for c in full) and any(c["P"] > 1 and c["S"] % c["P"] for c in full)
    assert any(c["G"] == 1 and c["path"] == "v4" for c in full) and any(c["G"] > 1 for c in full)
    assert any(c["path"] == "scalar" for c in full) and any(c["path"] == "scalar" and c["C"] > c["thr"] for c in full)
    assert any(c["doubled"] for c in full)
    assert [c["C"] for c in full if c["quads_over"]] == [4100]                             # FC2 with more quads than threads
    assert any(c["Cr"] > c["thr"] // 64 and c["Cr"] % (4 * (c["thr"] // 64)) for c in full)   # FC1: a second row in flight, and rows clamped to Cr - 1
    assert all(c["lds"] <= 64 * 1024 for c in se)
    # the mean stage alone (identity FCs): P == 1, P > 1 with a ragged subset, the scalar path
    probes = [c for c in se if c["probe"]]
    assert any(c["P"] == 1 and c["S"] > 1 for c in probes) and any(c["P"] > 1 and c["S"] % c["P"] for c in probes) and any(c["path"] == "scalar" for c in probes)


def test_relu6_clips_a_visible_share(listing):
    shares = [float(c["clip"]) for kind in ("dwt", "dwg") for c in cases_of(listing, kind) if c["act"] == "relu6"]
    assert len(shares) >= 10 and len(shares) == sum(c["act"] == "relu6" for kind in ("dwt", "dwg") for c in cases_of(listing, kind))
    assert min(shares) >= 0.01 and max(shares) <= 0.50, (min(shares), max(shares))


REF_CASES = ["t_k3s2_even", "t_k3s1_valid", "t_k5s2_ff", "t_k5s1_bf", "g_3x1_c8", "g_1x5_s12_c6", "m_hw513_c130", "se_c24_cr4_s3", "se_c6_cr3_s2_scalar"]


@pytest.mark.parametrize("name", REF_CASES)
def test_lab_reference_agrees_with_the_f64_oracle(lab, tmp_path, name):
    """The lab's fp64 loop nests against the project's independent oracle on the same case, built as a TFLite graph (the depthwise as a
    DEPTHWISE_CONV_2D, squeeze-excite as MEAN -> FC -> FC): two fp64 evaluations that differ in summation order only (at most 513 terms
    of magnitude <= scale: ~513 * 2^-53 ~ 6e-14) -> 1e-12 of the output scale."""
    from birdnet_go_amd import tflite_schema as S
    from birdnet_go_amd.tflite_build import GraphBuilder
    from oracle.interp import Interpreter
    r = subprocess.run([lab, "--ref-dump", name, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    meta = dict(ln.strip().split("=") for ln in open(tmp_path / "meta.txt"))
    mi = {k: int(v) for k, v in meta.items() if re.fullmatch(r"-?\d+", v)}
    f32 = lambda fn: np.fromfile(tmp_path / fn, np.float32)
    g = GraphBuilder(description="dwse lab case")
    i32 = lambda v: np.asarray(v, np.int32)

    def act(t, a, shape):
        if a == "swish":
            return g.op("MUL", [t, g.op("LOGISTIC", [t], shape)], shape, {})
        if a == "sigmoid":
            return g.op("LOGISTIC", [t], shape)
        return t
    fused = lambda a: {"relu": S.ACT_RELU, "relu6": S.ACT_RELU6}.get(a, S.ACT_NONE)
    B = mi["B"]
    if meta["kind"] == "dw":
        H, W, C, Ho, Wo = (mi[q] for q in ("H", "W", "C", "Ho", "Wo"))
        x = g.tensor([1, H, W, C], name="image")
        d = g.op("DEPTHWISE_CONV_2D", [x, g.const(f32("w.f32").reshape(1, mi["kh"], mi["kw"], C)), g.const(f32("b.f32"))], [1, Ho, Wo, C],
                 dict(padding=S.PAD_VALID if mi["valid"] else S.PAD_SAME, stride_w=mi["sw"], stride_h=mi["sh"], dilation_w_factor=1, dilation_h_factor=1,
                      depth_multiplier=1, fused_activation_function=fused(meta["act"])))
        y = act(d, meta["act"], [1, Ho, Wo, C])
        xin = f32("x.f32")
    elif meta["kind"] == "mean":
        x = g.tensor([1, mi["HW"], 1, mi["C"]], name="image")
        y = g.op("MEAN", [x, g.const(i32([1, 2]))], [1, mi["C"]], dict(keep_dims=0))
        xin = f32("x.f32")
    else:
        Sl, C, Cr = mi["S"], mi["C"], mi["Cr"]
        assert mi["HW"] == 32 * Sl                       # the slab sums / 32, exactly, are an image whose MEAN over S pixels is sums / HW
        x = g.tensor([1, Sl, 1, C], name="image")
        m = g.op("MEAN", [x, g.const(i32([1, 2]))], [1, C], dict(keep_dims=0))
        r1 = g.op("FULLY_CONNECTED", [m, g.const(f32("w1.f32").reshape(Cr, C)), g.const(f32("b1.f32"))], [1, Cr], dict(fused_activation_function=fused(meta["act1"])))
        r1 = act(r1, meta["act1"], [1, Cr])
        w2 = np.ascontiguousarray(f32("w2t.f32").reshape(Cr, C).T)
        y = g.op("FULLY_CONNECTED", [r1, g.const(w2), g.const(f32("b2.f32"))], [1, C], dict(fused_activation_function=fused(meta["act2"])))
        y = act(y, meta["act2"], [1, C])
        xin = f32("partial.f32") / np.float32(32)
    keep = {}
    Interpreter(g.finish([x], [y]), "f64").invoke(xin.reshape(B, -1), keep=keep)
    ref = np.asarray(keep[y])
    assert ref.dtype == np.float64
    got = np.fromfile(tmp_path / "y.f64", np.float64).reshape(ref.shape)
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max()) / scale
    print(f"{name}: lab fp64 reference vs oracle f64: {err:.3e} of the output scale {scale:.3g}")
    assert scale > 0 and err <= 1e-12, err


def _run(lab, env_extra):
    """One pass in one process with its own time limit (a pass is a few seconds: the host references dominate)."""
    env = dict(os.environ)
    env.pop("BNHIP_DW_PREFETCH", None)
    env.pop("BNHIP_SE_THREADS", None)
    env.update(env_extra)
    return subprocess.run([lab], capture_output=True, text=True, timeout=300, env=env)


def _check(r, want_cases, load_form):
    tail = "\n".join(r.stdout.splitlines()[-40:]) + r.stderr[-2000:]
    got = parse(r.stdout)
    fails = [ln for ln in r.stdout.splitlines() if ln.startswith("FAIL")]
    print("\n".join(ln for ln in r.stdout.splitlines() if ln.startswith("FORM ")))
    assert f"LOADFORM {load_form}" in r.stdout, tail
    assert got["failures"] == 0 and not fails, "\n".join(fails[:40])
    assert r.returncode == 0, tail
    assert got["ran"] == got["cases"] == want_cases, (got, want_cases)


@pytest.mark.gpu
def test_every_kernel_matches_fp64_on_the_device(gpu, lab, listing):
    """The default process runs the whole list (bf16 inputs of k_dwconv_t prefetched), the second one the bf16-input cases of
    k_dwconv_t row by row.  No retry; no second process after a first one that ended by a HIP error, a signal or its time limit
    (subprocess.run raises on the latter)."""
    want = parse(listing)["cases"]
    r1 = _run(lab, {})
    assert r1.returncode in (0, 1), "\n".join(r1.stdout.splitlines()[-40:]) + r1.stderr[-2000:]
    r2 = _run(lab, {"BNHIP_DW_PREFETCH": "0"})
    _check(r1, want, "prefetched")
    assert r2.returncode in (0, 1), "\n".join(r2.stdout.splitlines()[-40:]) + r2.stderr[-2000:]
    n16 = sum(c["in16"] for c in cases_of(listing, "dwt"))
    assert n16 >= 16
    _check(r2, n16, "rowwise")
    assert all("bf16-rowwise" in ln for ln in r2.stdout.splitlines() if ln.startswith("RUN "))
