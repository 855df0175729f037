"""Kernel-level exactness of the fused expand + depthwise family (csrc/expdw.hip), without a model: tools/ubench/expdw_lab drives
launch_expand_dw / launch_dwconv_lds WITH AN EXPLICIT SHAPE INDEX over a fixed case list - every tile shape in both orientations,
every arithmetic form the dispatcher can take on it - and holds every output element and every per-tile squeeze-excite sum to a plain
fp64 loop nest (gate: 4 x the error of a plain fp32 evaluation of the same case + 2^-22; DESIGN.md, "fused family: what is pinned per
form").  The model-level tests see these kernels only through logits, and only the instantiations the tuner picked that day.

Here: the coverage condition on the case list and the lab's own fp64 reference against the oracle run without a GPU; one pass of the
whole list runs on the device."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PIPE16 = [p + x for p in ("pipe16_kw24", "pipe16_kw32", "pipe16_ns2", "pipe16_ns3", "pipe16_ns5") for x in ("", "_xbf16")]
CHUNK_LOOP = ["sk16", "sk24", "sk32"]
# what every four-wave shape index must have run: the dispatcher's branches ...
FOUR_WAVE = (["f32_full", "f32_h8", "bx", "bx1", "copy"] + CHUNK_LOOP + PIPE16
             # ... the activations on both sides, bf16 storage, no sums buffer ...
             + ["acte_relu6", "acte_none", "actd_swish", "actd_relu6", "actd_none", "out_bf16", "copy_xbf16", "nosums"]
             # ... and the chunk loop of EVERY small-K instantiation, f32 and bf16 pipe alike: whole (a batch large enough that
             # B * tiles >= CUs / 2: the inter-chunk barrier, the deferred sums of chunk c - 1, the parameter prefetch, the operands
             # resident across chunks - the production path), cut into one-chunk parts (a small call) ...
             + [f + p for f in CHUNK_LOOP + PIPE16 for p in ("+parted", "+whole")]
             # ... and cut into parts of several chunks with a ragged last one (1 < cpp < chunks: five chunks as 2 + 2 + 1)
             + [f + "+parts" for f in CHUNK_LOOP + ["pipe16_ns3", "pipe16_ns5_xbf16"]])
EIGHT_WAVE = [f + "_nw8" + p for f in CHUNK_LOOP for p in ("", "+parted", "+whole", "+parts")]
STEM_SHAPES = (0, 1, 2, 3)
# (shape index, form) pairs that no layer can reach through launch_expand_dw / launch_dwconv_lds: none.  Every branch of the launchers'
# dispatch is keyed by (Cin, act_e, prec, image, stem) alone and every shape index is offered to each of them, except the eight-wave
# shapes (chunk-loop f32 form only, by expdw_shape_fits) and the stem (image orientation of the four 3 x 3 stride-1 shapes only) -
# both already excluded from the expectation below by construction.
UNREACHABLE = set()


def shape_table(listing):
    """The tile-shape table as the lab prints it (its copy is checked against the library's expdw_shape_slabs on every case):
    [(k, stride, tile rows, tile columns, footprint-row cap, waves)]; index i + n = entry i with rows and columns swapped."""
    rows = re.findall(r"^SHAPE (\d+) k=(\d+) s=(\d+) toh=(\d+) tow=(\d+) trh=(\d+) nw=(\d+)$", listing, re.M)
    assert [int(r[0]) for r in rows] == list(range(len(rows))) and len(rows) >= 22
    return [tuple(int(v) for v in r[1:]) for r in rows]


def expected_pairs(tiles):
    want, N = set(), len(tiles)
    for i in range(2 * N):
        nw = tiles[i % N][5]
        for f in (FOUR_WAVE if nw == 4 else EIGHT_WAVE):
            want.add((i, f))
        if i in STEM_SHAPES:
            want.add((i, "stem"))
    return want - UNREACHABLE


@pytest.fixture(scope="module")
def lab(built_lib, tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("expdw_lab") / "expdw_lab")
    libdir = os.path.dirname(built_lib)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "birdnet-go_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "ubench", "expdw_lab.cpp"), "-L", libdir, "-lbnhip", "-Wl,-rpath," + libdir],
                   check=True, capture_output=True, timeout=600)
    return exe


def parse(out):
    pairs = {(int(m.group(1)), m.group(2)) for m in re.finditer(r"^PAIR (\d+) (\S+) cases=(\d+)", out, re.M)}
    m = re.search(r"^SUMMARY (\{.*\})$", out, re.M)
    assert m, out[-2000:]
    return pairs, json.loads(m.group(1))


@pytest.fixture(scope="module")
def listing(lab):
    r = subprocess.run([lab, "--list"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_case_list_covers_every_shape_index_and_form(listing):
    pairs, summary = parse(listing)
    tiles = shape_table(listing)
    N = len(tiles)
    assert all(t[:2] == (3, 1) and t[5] == 4 for t in tiles[:4])          # the stem's shapes
    want = expected_pairs(tiles)
    missing = sorted(want - pairs)
    assert not missing, f"{len(missing)} (shape index, form) pairs have no case: {missing[:40]}"
    # nothing outside the vocabulary above (a new dispatcher branch must be added to the expectation, not slip past it)
    known = set(FOUR_WAVE) | set(EIGHT_WAVE) | {"stem"}
    assert {f for _, f in pairs} <= known, sorted({f for _, f in pairs} - known)
    assert {i for i, _ in pairs} == set(range(2 * N))
    assert summary["pairs"] == len(pairs) and summary["cases"] >= len(pairs) and summary["cus"] == 256
    # the geometry edges and the channel widths the list has to contain
    layers = [dict(kv.split("=") for kv in ln.split()[2:]) for ln in listing.splitlines() if ln.startswith("LAYER ")]
    assert {16, 20, 24, 32, 36, 40, 48, 64, 96, 128, 160} <= {int(l["Cin"]) for l in layers}
    cm = {int(l["Cmid"]) for l in layers}
    assert any(c % 32 == 0 for c in cm) and any(c % 32 == 4 for c in cm) and any(c % 32 == 28 for c in cm) and any(c >= 160 for c in cm)
    assert len({(l["k"], l["s"], l["H"], l["W"]) for l in layers}) >= 8
    assert any(int(l["s"]) == 2 and int(l["H"]) % 2 == 1 for l in layers) and any(int(l["s"]) == 2 and int(l["W"]) % 2 == 0 for l in layers)
    assert any(int(l["H"]) < 8 and int(l["W"]) < 8 for l in layers)                                   # smaller than any tile
    assert any(int(l["H"]) >= 8 * int(l["W"]) for l in layers) and any(int(l["W"]) >= 8 * int(l["H"]) for l in layers)   # tall-narrow, wide-flat
    assert {1} <= {int(l["B"]) for l in layers} and max(int(l["B"]) for l in layers) >= 128


def test_relu6_clips_a_visible_share(listing):
    shares = [float(v) for ln in listing.splitlines() if ln.startswith("LAYER ") for v in re.findall(r"clip_[ed]=(\S+)", ln) if float(v) >= 0]
    assert len(shares) >= 50
    assert min(shares) >= 0.01 and max(shares) <= 0.50, (min(shares), max(shares))


REF_CASES = ["k3s1_ragged/c20x36/B1", "k5s1_ragged/c24x60/B2", "k3s2_oddeven/c36x36/B2", "k5s2_oddeven/c32x64_er6/B2", "k3s2_evenodd/c24x36_en/B2",
             "k5s2_flat/c48x60_bx/B2", "k3s1_tiny/c24x60_p1/B1", "k5s1_tall/copy100_r6/B2", "stem_ragged/stem32/B2", "stem_flat/stem64_r6/B2"]


@pytest.mark.parametrize("name", REF_CASES)
def test_lab_reference_agrees_with_the_f64_oracle(lab, tmp_path, name):
    """The lab's fp64 loop nest against the project's independent oracle on the same block, built as a TFLite graph: two fp64 evaluations
    that differ in summation order only (at most 160 * 25 terms of magnitude <= scale: ~4000 * 2^-53 ~ 5e-13) -> 1e-12 of the output scale."""
    from birdnet_go_amd import tflite_schema as S
    from birdnet_go_amd.tflite_build import GraphBuilder
    from oracle.interp import Interpreter
    r = subprocess.run([lab, "--ref-dump", name, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    meta = dict(ln.strip().split("=") for ln in open(tmp_path / "meta.txt"))
    mi = {k: int(v) for k, v in meta.items() if k not in ("act_e", "act_d")}
    f32 = lambda fn: np.fromfile(tmp_path / fn, np.float32)
    B, H, W, Cin, Cm, k, s, Ho, Wo = (mi[q] for q in ("B", "H", "W", "Cin", "Cmid", "k", "s", "Ho", "Wo"))
    g = GraphBuilder(description="expdw lab block")

    def act(t, name_, shape):
        if name_ == "swish":
            return g.op("MUL", [t, g.op("LOGISTIC", [t], shape)], shape, {})
        return t
    fused = lambda a: S.ACT_RELU6 if a == "relu6" else S.ACT_NONE
    conv = lambda st: dict(padding=S.PAD_SAME, stride_w=st, stride_h=st, dilation_w_factor=1, dilation_h_factor=1)
    if mi["stem"]:
        x = g.tensor([1, mi["Hin"], mi["Win"], 2], name="image")
        t = g.op("CONV_2D", [x, g.const(f32("we.f32").reshape(Cm, 3, 3, 2)), g.const(f32("be.f32"))], [1, H, W, Cm],
                 dict(conv(2), fused_activation_function=fused(meta["act_e"])))
        t = act(t, meta["act_e"], [1, H, W, Cm])
        xin = f32("x.f32").reshape(B, mi["Hin"], mi["Win"], 2)
    elif mi["copy"]:
        x = t = g.tensor([1, H, W, Cm], name="image")
        xin = f32("x.f32").reshape(B, H, W, Cm)
    else:
        x = g.tensor([1, H, W, Cin], name="image")
        t = g.op("CONV_2D", [x, g.const(f32("we.f32").reshape(Cm, 1, 1, Cin)), g.const(f32("be.f32"))], [1, H, W, Cm],
                 dict(conv(1), fused_activation_function=fused(meta["act_e"])))
        t = act(t, meta["act_e"], [1, H, W, Cm])
        xin = f32("x.f32").reshape(B, H, W, Cin)
    d = g.op("DEPTHWISE_CONV_2D", [t, g.const(f32("wd.f32").reshape(1, k, k, Cm)), g.const(f32("bd.f32"))], [1, Ho, Wo, Cm],
             dict(conv(s), depth_multiplier=1, fused_activation_function=fused(meta["act_d"])))
    y = act(d, meta["act_d"], [1, Ho, Wo, Cm])
    keep = {}
    Interpreter(g.finish([x], [y]), "f64").invoke(xin.reshape(B, -1), keep=keep)
    ref = np.asarray(keep[y])
    assert ref.dtype == np.float64
    got = np.fromfile(tmp_path / "y.f64", np.float64).reshape(ref.shape)
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max()) / scale
    print(f"{name}: lab fp64 reference vs oracle f64: {err:.3e} of the output scale {scale:.3g}")
    assert scale > 0 and err <= 1e-12, err


@pytest.mark.gpu
def test_every_fused_form_matches_fp64_on_the_device(gpu, lab, listing):
    """One process, one pass over the whole list (about 6300 launches of small layers: seconds on the device, most of the 80 s is the host
    references); a non-zero exit fails with the lab's last lines - no retry."""
    want_pairs, want = parse(listing)
    r = subprocess.run([lab], capture_output=True, text=True, timeout=900)
    tail = "\n".join(r.stdout.splitlines()[-40:]) + r.stderr[-2000:]
    assert r.returncode == 0, tail
    pairs, got = parse(r.stdout)
    fails = [ln for ln in r.stdout.splitlines() if ln.startswith("FAIL")]
    assert got["failures"] == 0 and not fails, "\n".join(fails[:40])
    assert got["cus"] == 256 or pairs >= expected_pairs(shape_table(listing))        # (another CU count moves cases between "+parted", "+parts" and "+whole")
    assert got["ran"] == got["cases"] == want["cases"], (got, want)
    if got["cus"] == 256:
        assert pairs == want_pairs, sorted(pairs ^ want_pairs)[:40]
    print("\n".join(ln for ln in r.stdout.splitlines() if ln.startswith("FORM ")))
