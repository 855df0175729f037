"""Cost of one species occurrence heat-map at the API's maximum grid (50 000 cells x 48 weeks = 2.4 M model rows,
internal/api/v2/analytics/heatmap.go:30-36) on the range-filter stand-ins, three ways:
  (a) today's path for a host that plugs this library in as the range filter - computeHeatmapGrid (heatmap.go:315-368):
      host.RangeFilter.predict_batch over each week's rows in chunks of 512 (BatchRangeFilterInference, orchestrator.go:1846-1883)
      and of 4096 (heatmapOptBatchSize), every species copied back and the one column kept on the host;
  (b) one bnhip_range_heatmap call (host.RangeFilter.heatmap);
  (c) a torch-CPU restatement of the same MLP (TorchMLP below, 16 threads, chunks of 4096 rows) - a RESTATEMENT, not ONNX
      Runtime - timed over the first --cpu-weeks weeks and scaled to the 48 (its rows cost the same every week).
Stand-ins: 3 -> 64 -> 128 -> 6522 (the v2.4 meta-model's output width) and 3 -> 512 -> 300 -> 12000 (the published geomodel's
width; hidden widths chosen only so the fp16 constants weigh about its 7.48 MB).  Host clock around calls that end in a
synchronise; one warm-up call per leg (one week for (a), one chunk for (c)).  Every leg's column is compared with (b).  Prints one JSON line.

    python tools/heatmap_rate.py [--cells 50000] [--weeks 48] [--species 4321] [--rounds 3] [--cpu-weeks 2] [--models 6522,12000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import birdnet_go_amd  # noqa: E402,F401
from birdnet_go_amd import host, synth_model as sm  # noqa: E402

MODELS = {6522: (64, 128), 12000: (512, 300)}


def grid_coords(n_cells):
    """A grid of the handler's form with n_cells cells: 250 x (n_cells / 250) at 0.5 degrees from (-60, -150)."""
    cols = 250
    rows = (n_cells + cols - 1) // cols
    _, _, c = host.heatmap_grid(-60.0, -60.0 + rows * 0.5, -150.0, -150.0 + cols * 0.5, 0.5)
    return c[:n_cells]


def week_rows(coords, week):
    r = np.empty((coords.shape[0], 3), np.float32)
    r[:, :2] = coords
    r[:, 2] = np.float32(week)
    return r


def leg_a(rf, coords, weeks, species, chunk):
    n = coords.shape[0]
    out = np.empty((weeks, n), np.float32)
    for wi in range(weeks):
        rows = week_rows(coords, wi + 1)
        for c0 in range(0, n, chunk):
            k = min(chunk, n - c0)
            out[wi, c0:c0 + k] = rf.predict_batch(rows[c0:c0 + k].reshape(-1), k).reshape(k, -1)[:, species]
    return out


class TorchMLP:
    """The stand-in's graph restated on torch-CPU: FULLY_CONNECTED layers (fp16 constants widened, as DEQUANTIZE does), fused
    RELU, trailing LOGISTIC.  A RESTATEMENT, not ONNX Runtime."""

    def __init__(self, blob):
        import torch
        from oracle.tflite_reader import read_model
        m = read_model(blob)
        deq = {op.outputs[0]: op.inputs[0] for op in m.ops if op.name == "DEQUANTIZE"}
        const = lambda t: torch.from_numpy(np.asarray(m.tensors[deq.get(t, t)].data, np.float32).copy())
        self.layers, self.sigmoid = [], False
        for op in m.ops:
            if op.name == "FULLY_CONNECTED":
                self.layers.append((const(op.inputs[1]), const(op.inputs[2]), op.opts.get("act", 0)))
            elif op.name == "LOGISTIC":
                self.sigmoid = True

    def predict(self, rows):
        import torch
        t = torch.from_numpy(rows)
        for w, b, act in self.layers:
            t = torch.addmm(b, t, w.T)
            if act == 1:
                t = torch.relu(t)
        return (torch.sigmoid(t) if self.sigmoid else t).numpy()


def leg_c(tc, coords, weeks, species, chunk=4096):
    import torch
    n = coords.shape[0]
    out = np.empty((weeks, n), np.float32)
    with torch.inference_mode():
        for wi in range(weeks):
            rows = week_rows(coords, wi + 1)
            for c0 in range(0, n, chunk):
                out[wi, c0:c0 + chunk] = tc.predict(rows[c0:c0 + chunk])[:, species]
    return out


def timed(fn, rounds, warm=None):
    (warm or fn)()                                                   # warm-up
    ts, res = [], None
    for _ in range(rounds):
        t0 = time.perf_counter()
        res = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--weeks", type=int, default=48)
    ap.add_argument("--species", type=int, default=4321)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--a-rounds", type=int, default=1)
    ap.add_argument("--cpu-weeks", type=int, default=2)
    ap.add_argument("--models", default="6522,12000")
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--max-batch", type=int, default=4096)
    a = ap.parse_args()
    host.init()                                                      # no device: a loud error, not a fallback
    coords = grid_coords(a.cells)
    res = {"tool": "heatmap_rate", "cells": a.cells, "weeks": a.weeks, "rows": a.cells * a.weeks, "species": a.species,
           "max_batch": a.max_batch, "models": {}}
    ok = True
    for width in [int(v) for v in a.models.split(",")]:
        blob = sm.build_dense_model([3, *MODELS[width], width], final_sigmoid=True, fp16_weights=True, input_scale=[90.0, 180.0, 48.0])
        rf = host.RangeFilter(blob, max_batch=a.max_batch)
        r = {"dims": [3, *MODELS[width], width], "heatmap_tail": rf._clf.describe()["heatmap_tail"]}
        ms, best, hb = timed(lambda: rf.heatmap(coords, a.species, 1, a.weeks), a.rounds)
        r["b_range_heatmap_ms"], r["b_range_heatmap_min_ms"] = round(ms, 2), round(best, 2)
        r["b_rows_per_s"] = round(a.cells * a.weeks / (ms / 1e3))
        print(f"[heatmap_rate] {width}: leg b {ms:.1f} ms", file=sys.stderr, flush=True)
        if "a" in a.legs:
            for chunk in (512, 4096):
                ms, best, ha = timed(lambda: leg_a(rf, coords, a.weeks, a.species, chunk), a.a_rounds,
                                     lambda: leg_a(rf, coords, 1, a.species, chunk))
                r[f"a_predict_batch_{chunk}_ms"] = round(ms, 1)
                r[f"a_predict_batch_{chunk}_calls"] = a.weeks * ((a.cells + chunk - 1) // chunk)
                r[f"a_predict_batch_{chunk}_d2h_bytes"] = a.weeks * a.cells * width * 4
                r[f"speedup_b_over_a_{chunk}"] = round(ms / r["b_range_heatmap_ms"], 1)
                d = float(np.abs(ha - hb).max())
                r[f"max_abs_diff_a_{chunk}_b"] = d
                print(f"[heatmap_rate] {width}: leg a/{chunk} {ms:.0f} ms", file=sys.stderr, flush=True)
                ok = ok and d <= 1e-6
        if "c" in a.legs:
            import torch
            torch.set_num_threads(16)
            tc = TorchMLP(blob)
            cw = min(a.cpu_weeks, a.weeks)
            ms, best, hc = timed(lambda: leg_c(tc, coords, cw, a.species), 1, lambda: leg_c(tc, coords[:4096], 1, a.species))
            r["c_torch_cpu_restatement_weeks_timed"] = cw
            r["c_torch_cpu_restatement_ms_scaled"] = round(ms * a.weeks / cw, 1)
            r["speedup_b_over_c"] = round(r["c_torch_cpu_restatement_ms_scaled"] / r["b_range_heatmap_ms"], 1)
            d = float(np.abs(hc - hb[:cw]).max())
            r["max_abs_diff_c_b"] = d
            ok = ok and d <= 2e-6
        rf.close()
        res["models"][str(width)] = r
        print(json.dumps({str(width): r}), file=sys.stderr, flush=True)
    res["columns_agree"] = ok
    print(json.dumps(res))
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
