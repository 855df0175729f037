"""Species occurrence heat-map grids (bnhip_range_heatmap, RangeFilter.heatmap, heatmap_grid, the Go shim's ComputeGrid): the
grid request of HeatmapInferenceService.ComputeGridWithBinding (internal/classifier/heatmap_service.go:143-420) on the device.
CPU: the surface, every refusal by its reason on plan-only handles, which tail form a plan gets, the grid formula.  GPU: against
the oracles and predict_batch's column, on the pruned and the gather tail."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from birdnet_go_amd import host, onnx_build as ob, synth_model as sm, tflite_schema as S
from birdnet_go_amd.tflite_build import GraphBuilder
from oracle import onnx_interp
from oracle.interp import Interpreter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPDIR = os.path.join(ROOT, "birdnet-go_amd", "go", "internal", "inference", "hip")
SCALE = [90.0, 180.0, 48.0]


def _lib():
    lib = host.load_library()
    lib.bnhip_range_heatmap.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


def standin(n_out=6522, hidden=(64, 128)):
    """The range-filter stand-in of test_range_filter_fp16_batch: fp16 constants behind DEQUANTIZE, in-graph sigmoid."""
    return sm.build_dense_model([3, *hidden, n_out], final_sigmoid=True, fp16_weights=True, input_scale=SCALE)


def identity_model(trailing_max=False):
    """[lat, lon, week] -> the same three values: a dense layer with identity weights and zero bias.  With trailing_max an
    elementwise MAXIMUM with -1e4 follows it, a tail the pruning rule excludes (same values, gather form)."""
    g = GraphBuilder(description="identity range filter")
    x = g.tensor([1, 3], name="INPUT")
    t = g.op("FULLY_CONNECTED", [x, g.const(np.eye(3, dtype=np.float32), "w"), g.const(np.zeros(3, np.float32), "b")], [1, 3],
             dict(fused_activation_function=S.ACT_NONE), name="fc")
    if trailing_max:
        t = g.op("MAXIMUM", [t, g.const(np.full(3, -1e4, np.float32), "floor")], [1, 3], {}, name="OUT")
    return g.finish([x], [t])


def onnx_dense(final="Sigmoid", extra_mul=False, dims=(3, 48, 96, 500)):
    """ONNX Gemm (+ Relu) layers and a final activation; extra_mul puts an elementwise Mul behind it."""
    rng = np.random.default_rng(5)
    b = ob.OnnxBuilder()
    t = b.input("x", ["N", dims[0]])
    for li in range(len(dims) - 1):
        w = (rng.standard_normal((dims[li + 1], dims[li])) / np.sqrt(dims[li])).astype(np.float32)
        if li == 0:
            w = (w / np.asarray(SCALE, np.float32)[None, :]).astype(np.float32)
        bias = (rng.standard_normal(dims[li + 1]) * 0.1).astype(np.float32)
        t = b.node("Gemm", [t, b.init(w), b.init(bias)], alpha=1.0, beta=1.0, transB=1)
        if li < len(dims) - 2:
            t = b.node("Relu", [t])
    t = b.node(final, [t], axis=-1) if final == "Softmax" else b.node(final, [t])
    if extra_mul:
        t = b.node("Mul", [t, b.init(np.full(dims[-1], 0.5, np.float32))])
    b.output(t, ["N", dims[-1]])
    return b.finish()


def grid_rows(coords, weeks, stride):
    """The model rows of a grid request in result order: row wi * n_cells + c = [lat_c, lon_c, 1 + wi * stride]."""
    n = coords.shape[0]
    rows = np.empty((weeks * n, 3), np.float32)
    for wi in range(weeks):
        rows[wi * n:(wi + 1) * n, :2] = coords
        rows[wi * n:(wi + 1) * n, 2] = np.float32(1 + wi * stride)
    return rows


def tail(blob, **kw):
    c = host.HipClassifier(blob, plan_only=True, **kw)
    d = c.describe()["heatmap_tail"]
    c.close()
    return d


# ------------------------------------------------------------------------------------------------ CPU
def test_symbol_exported_and_declared(built_lib):
    assert hasattr(C.CDLL(built_lib), "bnhip_range_heatmap") and "bnhip_range_heatmap" in host.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "bnhip.h")).read()
    assert re.search(r"int bnhip_range_heatmap\(bnhip_model\* m, const float\* coords, int n_cells, int species,\s*"
                     r"int stride, int total_weeks, float\* result\);", hdr)


def test_refusals_by_reason(built_lib):
    lib = _lib()
    rf = host.HipClassifier(standin(n_out=40), plan_only=True)
    coords = np.zeros(2 * 8, np.float32)
    res = np.full(64, 7.0, np.float32)
    h, cp, rp = rf._h, coords.ctypes.data, res.ctypes.data

    def refused(rc, reason):
        assert rc == host.E_INVALID, rc
        assert reason in lib.bnhip_last_error().decode(), (reason, lib.bnhip_last_error())
        assert (res == 7.0).all()

    refused(lib.bnhip_range_heatmap(None, cp, 8, 0, 1, 1, rp), "NULL argument")
    refused(lib.bnhip_range_heatmap(h, None, 8, 0, 1, 1, rp), "NULL argument")
    refused(lib.bnhip_range_heatmap(h, cp, 8, 0, 1, 1, None), "NULL argument")
    for n_cells, stride, weeks in ((0, 1, 1), (-3, 1, 1), (8, 0, 1), (8, -2, 1), (8, 1, 0), (8, 1, -48)):
        refused(lib.bnhip_range_heatmap(h, cp, n_cells, 0, stride, weeks, rp), "must be positive")
    for sp in (-1, 40, 1 << 20):
        refused(lib.bnhip_range_heatmap(h, cp, 8, sp, 1, 1, rp), "out of range [0, 40)")
    refused(lib.bnhip_range_heatmap(h, cp, (1 << 30), 0, 1, 48, rp), "overflows")
    refused(lib.bnhip_range_heatmap(h, cp, (1 << 31) - 1, 0, 24, 48, rp), "overflows")      # 2 weeks
    refused(lib.bnhip_range_heatmap(h, cp, 8, 0, 1, 48, rp), "plan-only")
    rf.close()
    wide = host.HipClassifier(sm.build_dense_model([4, 8, 5]), plan_only=True)
    refused(lib.bnhip_range_heatmap(wide._h, cp, 8, 0, 1, 1, rp), "must take 3 inputs")
    wide.close()
    multi = host.HipClassifier(standin(n_out=40), plan_only=True, devices=[0, 0])
    refused(lib.bnhip_range_heatmap(multi._h, cp, 8, 0, 1, 1, rp), "single-device")
    multi.close()


def test_tail_rule():
    assert tail(standin()) == "pruned"                                   # FC + trailing LOGISTIC folded, fp16 DEQUANTIZE constants
    assert tail(standin(n_out=12000, hidden=(512, 300))) == "pruned"
    assert tail(sm.build_dense_model([3, 16, 9])) == "pruned"            # no activation at all
    assert tail(identity_model()) == "pruned"                            # the dense layer reads the model input itself
    assert tail(onnx_dense()) == "pruned"                                # ONNX Gemm + Sigmoid
    blob, _ = ob.build_dense_head([3, 32, 20], style="gemm", final="Sigmoid")
    assert tail(blob) == "pruned"                                        # ... behind an Identity
    assert tail(onnx_dense(final="Softmax")) == "gather"
    assert tail(onnx_dense(extra_mul=True)) == "gather"
    assert tail(identity_model(trailing_max=True)) == "gather"
    assert tail(standin(), precision="bf16") == "gather"                 # bf16 engines run the whole plan


def _handler_grid(south, north, west, east, res):
    """internal/api/v2/analytics/heatmap.go:212-219 (heatmapGridDimensions) and :315-330, statement for statement."""
    rows = max(1, int(math.ceil((north - south) / res)))
    cols = max(1, int(math.ceil((east - west) / res)))
    out = []
    for r in range(rows):
        lat = np.float32(south + (float(r) + 0.5) * res)
        for c in range(cols):
            out.append((lat, np.float32(west + (float(c) + 0.5) * res)))
    return rows, cols, np.array(out, np.float32).reshape(-1, 2)


@pytest.mark.parametrize("ext", [(40.1, 58.55, -5.2, 6.1, 0.5), (-33.37, -12.01, 112.9, 153.63, 0.3), (10.0, 10.05, 20.0, 20.0, 0.1),
                                 (-89.95, 89.95, -179.9, 179.9, 5.0), (1.0 / 3, 7.0 / 3, -2.0 / 7, 5.0 / 7, 0.1)])
def test_heatmap_grid_is_the_handler_formula(ext):
    rows, cols, coords = host.heatmap_grid(*ext)
    r2, c2, want = _handler_grid(*ext)
    assert (rows, cols) == (r2, c2) and coords.dtype == np.float32 and coords.shape == (rows * cols, 2)
    assert np.array_equal(coords, want)


# ------------------------------------------------------------------------------------------------ Go shim (CPU)
def test_go_shim_carries_compute_grid(tmp_path):
    src = open(os.path.join(HIPDIR, "backend_hip.go")).read()
    stub = open(os.path.join(HIPDIR, "stub_nohip.go")).read()
    sig = "func (r *RangeFilter) ComputeGrid(coords []float32, totalCells, speciesIdx, stride, totalWeeks int, result []float32) error"
    assert sig in src
    assert "func (*RangeFilter) ComputeGrid([]float32, int, int, int, int, []float32) error" in stub
    body = src[src.index(sig):]
    body = body[:body.index("\n}\n")]
    assert "runtime.LockOSThread()" in body and "defer runtime.UnlockOSThread()" in body
    for check in ("len(coords) != totalCells*2", "stride <= 0 || totalWeeks <= 0", "len(result) < weeks*totalCells",
                  "speciesIdx < 0 || speciesIdx >= r.c.nClasses", "C.bnbind_range_heatmap("):
        assert check in body, check
    assert 'BN_RESOLVE(range_heatmap, "bnhip_range_heatmap")' in src
    # the preamble's function-pointer type is the header's declaration: assigning one to the other compiles warning-free
    td = re.search(r"typedef int\s+\(\*fn_range_heatmap\)\([^;]*\);", src).group(0)
    (tmp_path / "t.c").write_text(f'#include "bnhip.h"\n{td}\nint probe(void);\n'
                                  "int probe(void) { fn_range_heatmap f = bnhip_range_heatmap; return f != 0; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-Werror=incompatible-pointer-types", "-c",
                           "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t.o")])


# ------------------------------------------------------------------------------------------------ GPU
GRID = (40.1, 58.55, -5.2, 6.1, 0.5)          # 37 x 23 = 851 cells: a multiple of no chunk size used here


@pytest.fixture(scope="module")
def grid():
    rows, cols, coords = host.heatmap_grid(*GRID)
    assert (rows, cols) == (37, 23)
    return coords


@pytest.fixture(scope="module")
def rf6522(gpu):
    blob = standin()
    rf = host.RangeFilter(blob, max_batch=256)
    yield blob, rf
    rf.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 4, 48])
def test_standin_against_oracle_and_predict(rf6522, grid, stride):
    blob, rf = rf6522
    weeks = (48 + stride - 1) // stride
    rows = grid_rows(grid, weeks, stride)
    rng = np.random.default_rng(stride)
    pick = np.sort(rng.choice(rows.shape[0], min(rows.shape[0], 1500), replace=False))
    ref = Interpreter(blob).invoke(rows[pick])[0]
    pred = rf.predict_batch(rows[pick].reshape(-1), pick.size).reshape(pick.size, -1)
    for sp in (0, 3001, 6521):
        got = rf.heatmap(grid, sp, stride=stride, total_weeks=48)
        assert got.shape == (weeks, grid.shape[0]) and np.isfinite(got).all()
        flat = got.reshape(-1)[pick]
        assert np.abs(flat - ref[:, sp]).max() <= 2e-6, sp
        assert np.abs(flat - pred[:, sp]).max() <= 1e-6, sp


@pytest.mark.gpu
@pytest.mark.parametrize("trailing_max", [False, True])
def test_rows_are_assembled_exactly(gpu, grid, trailing_max):
    """Identity model: the heat-map of output 0 / 1 / 2 is the latitude / longitude / week of every row - the row layout, the
    week sequence 1 + wi * stride and the [week][cell] result layout, bit for bit, on the pruned and on the gather tail."""
    blob = identity_model(trailing_max)
    rf = host.RangeFilter(blob, max_batch=64)
    assert rf._clf.describe()["heatmap_tail"] == ("gather" if trailing_max else "pruned")
    weeks = 10                                                    # ceil(48 / 5)
    want = grid_rows(grid, weeks, 5).reshape(weeks, grid.shape[0], 3)
    for k in range(3):
        got = rf.heatmap(grid, k, stride=5, total_weeks=48)
        assert np.array_equal(got, want[:, :, k]), k
    rf.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_batch", [64, 4096])
def test_handle_geometry(gpu, grid, max_batch):
    blob = standin(n_out=700)
    rf = host.RangeFilter(blob, max_batch=max_batch)
    got = rf.heatmap(grid, 699, stride=2, total_weeks=48)
    rows = grid_rows(grid, 24, 2)
    pick = np.arange(0, rows.shape[0], 7)
    ref = Interpreter(blob).invoke(rows[pick])[0][:, 699]
    assert np.abs(got.reshape(-1)[pick] - ref).max() <= 2e-6
    pred = rf.predict_batch(rows[pick].reshape(-1), pick.size).reshape(pick.size, -1)[:, 699]
    assert np.abs(got.reshape(-1)[pick] - pred).max() <= 1e-6
    rf.close()


@pytest.mark.gpu
@pytest.mark.parametrize("final,extra_mul", [("Softmax", False), ("Sigmoid", True)])
def test_gather_tail(gpu, grid, final, extra_mul):
    blob = onnx_dense(final=final, extra_mul=extra_mul)
    rf = host.RangeFilter(blob, max_batch=64)
    assert rf._clf.describe()["heatmap_tail"] == "gather"
    got = rf.heatmap(grid, 123, stride=3, total_weeks=48)
    rows = grid_rows(grid, 16, 3)
    ref = onnx_interp.run(blob, rows)[0][:, 123]
    assert np.abs(got.reshape(-1) - ref).max() <= 2e-6
    # one week, n_cells == max_batch: the chunk is the same set of rows as one predict call - bit-identical
    cells = grid[100:164]
    one = rf.heatmap(cells, 123, stride=1, total_weeks=1)
    pred = rf.predict_batch(grid_rows(cells, 1, 1).reshape(-1), 64).reshape(64, -1)
    assert np.array_equal(one[0], pred[:, 123])
    rf.close()


@pytest.mark.gpu
def test_onnx_standin_against_onnx_oracle(gpu, grid):
    blob = onnx_dense()
    rf = host.RangeFilter(blob, max_batch=512)
    assert rf._clf.describe()["heatmap_tail"] == "pruned"
    rows = grid_rows(grid, 12, 4)
    ref = onnx_interp.run(blob, rows)[0]
    for sp in (0, 250, 499):
        got = rf.heatmap(grid, sp, stride=4, total_weeks=48)
        assert np.abs(got.reshape(-1) - ref[:, sp]).max() <= 2e-6, sp
    rf.close()


@pytest.mark.gpu
def test_published_width_standin(gpu, grid):
    """12 000 outputs with fp16 constants of about the published geomodel's 7.48 MB (BirdNET+_Geomodel_V3.0.2_Global_12K_FP16,
    model_catalog.go:504-575).  That file's architecture is unknown: the hidden widths 512 / 300 are chosen for the size only."""
    blob = standin(n_out=12000, hidden=(512, 300))
    n16 = 3 * 512 + 512 + 512 * 300 + 300 + 300 * 12000 + 12000
    assert 7.3e6 < 2 * n16 < 7.7e6
    rf = host.RangeFilter(blob, max_batch=4096)
    assert rf.num_species() == 12000 and rf._clf.describe()["heatmap_tail"] == "pruned"
    rows = grid_rows(grid, 48, 1)
    pick = np.random.default_rng(9).choice(rows.shape[0], 600, replace=False)
    ref = Interpreter(blob).invoke(rows[pick])[0]
    for sp in (0, 7777, 11999):
        got = rf.heatmap(grid, sp)
        assert got.shape == (48, grid.shape[0])
        assert np.abs(got.reshape(-1)[pick] - ref[:, sp]).max() <= 2e-6, sp
    rf.close()


@pytest.mark.gpu
def test_failed_call_changes_nothing(rf6522, grid):
    blob, rf = rf6522
    lib = _lib()
    res = np.full(grid.shape[0], 3.0, np.float32)
    for sp in (-1, 6522):
        rc = lib.bnhip_range_heatmap(rf._clf._h, grid.ctypes.data, grid.shape[0], sp, 48, 48, res.ctypes.data)
        assert rc == host.E_INVALID and (res == 3.0).all()
    with pytest.raises(host.HipError, match="out of range"):
        rf.heatmap(grid, 6522)
    pts = grid_rows(grid[:40], 1, 1)
    assert np.abs(rf.predict_batch(pts.reshape(-1), 40).reshape(40, -1) - Interpreter(blob).invoke(pts)[0]).max() < 2e-6
    rc = lib.bnhip_range_heatmap(rf._clf._h, grid.ctypes.data, grid.shape[0], 17, 48, 48, res.ctypes.data)
    assert rc == 1
    assert np.abs(res - Interpreter(blob).invoke(grid_rows(grid, 1, 48))[0][:, 17]).max() <= 2e-6
