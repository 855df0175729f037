"""Detection events of one long recording on the full synthetic model, three ways (DESIGN section 9 "File analysis: detection events"):
  (a) one bnhip_analyze_pcm_events call: the rows stay on the device and the event tail runs behind the last chunk;
  (b) bnhip_analyze_pcm with every row brought down, then the rule on the host (tests/evref.py, the restatement the tests pin to);
  (c) bnhip_analyze_pcm alone: the floor, what the call costs before anyone merges anything.
The legs run in one process, alternated round by round, host clock around calls that end in a synchronise; medians over --rounds
after one warm-up of each, [min, max] beside them.  (a) must equal (b): np.array_equal, asserted.  --parent-lib names a library built
from the parent commit: leg (c) then runs on it too, alternated with the others ("floor_parent").  Also a burst of many short
recordings, and the tail alone (bnhip_detection_events) over a seeded million rows, so that the sort has real volume.  The filter's
thresholds come from the rows of the warm-up: the median confidence for every class, the most frequent class as the veto class
(heard above the 90th percentile of its confidences), a 15 s hold and the reference's level 3.  --floor-only runs leg (c) alone on
both libraries: with BNHIP_LIB naming the parent's and --parent-lib this one the two handles swap places, which tells a difference
between the libraries from one between the first and the second handle of a process; without --parent-lib it runs on the one
library BNHIP_LIB names, for processes alternated from outside.  Prints one JSON line.

    python tools/analyze_events_rate.py [--seconds 3600] [--overlaps 0,2.5] [--rounds 3] [--max-batch 256] [--parent-lib PATH]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import birdnet_go_amd  # noqa: E402,F401
from birdnet_go_amd import host, synth_model as sm, wav  # noqa: E402
import evref  # noqa: E402
from analyze_rate import CLIP, RATE, recording  # noqa: E402

NEG_INF = float("-inf")


def stats(ts):
    return {"median_ms": round(float(np.median(ts)), 2), "min_ms": round(min(ts), 2), "max_ms": round(max(ts), 2)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def filter_from(rows, n_classes, hop, overlap):
    thr = np.full(n_classes, np.float32(np.median(rows["confidence"])), np.float32)
    veto = np.zeros(n_classes, np.uint8)
    heard = int(np.bincount(rows["class_index"], minlength=n_classes).argmax())
    veto[heard] = 1
    veto_thr = np.float32(np.quantile(rows["confidence"][rows["class_index"] == heard], 0.9))
    return host.EventTables(thr, veto, float(veto_thr), max(1, math.ceil(15.0 * RATE / hop)), host.event_min_count(3, overlap),
                            host.EVENTS_KEEP_DROPPED)


def legs(c, parent, raw, lengths, hop, min_tail, k, overlap, rounds, floor_only=False):
    def rows_down(clf=c):
        return clf.analyze_pcm(raw, 16, lengths, hop, min_tail, k=k, threshold=NEG_INF)[0]

    rows = rows_down()                                                   # warm-up of (b) / (c), and what the filter is made from
    if floor_only:
        same = parent is None or rows_down(parent).tobytes() == rows.tobytes()
        ts = {"c_rows_call_floor": []} if parent is None else {"c_rows_call_floor": [], "floor_parent": []}
        for _ in range(rounds):
            ts["c_rows_call_floor"].append(timed(rows_down)[1])
            if parent is not None:
                ts["floor_parent"].append(timed(lambda: rows_down(parent))[1])
        r = {"hop": hop, "recordings": len(lengths), "rows": int(rows.size), "rows_equal": same, "rows_crc": int(np.frombuffer(rows.tobytes(), np.uint32).sum())}
        r.update({name: stats(t) for name, t in ts.items()})
        return r, same
    flt = filter_from(rows, c.num_species(), hop, overlap)

    def a():
        return c.analyze_pcm_events(raw, 16, lengths, hop, flt, min_tail, k=k)

    def b():
        return evref.events(rows_down(), flt)

    got, want = a(), b()                                                 # warm-up of (a) and of the restatement; the comparison
    same = bool(np.array_equal(got, want))
    todo = [("a_events_call", a), ("b_rows_down_then_host", b), ("c_rows_call_floor", rows_down)]
    if parent is not None:
        rows_down(parent)
        todo.append(("floor_parent", lambda: rows_down(parent)))
    ts = {name: [] for name, _ in todo}
    host_rule = []
    for _ in range(rounds):
        for name, fn in todo:
            ts[name].append(timed(fn)[1])
        host_rule.append(timed(lambda: evref.events(rows, flt))[1])
    r = {"hop": hop, "recordings": len(lengths), "rows": int(rows.size), "rows_bytes_over_pcie_saved": int(rows.nbytes), "events": int(got.size),
         "events_bytes": int(got.nbytes), "events_by_status": [int((got["status"] == s).sum()) for s in (0, 1, 2)],
         "hold_windows": flt.hold_windows, "min_count": flt.min_count, "a_equals_b": same, "host_rule_alone": stats(host_rule)}
    r.update({name: stats(t) for name, t in ts.items()})
    return r, same


def tail_alone(rounds, n=1_000_000, n_rec=200, n_classes=100, n_windows=500):
    rng = np.random.default_rng(25)
    rows = np.zeros(n, host.DETECTION)
    rows["recording"], rows["window"] = rng.integers(0, n_rec, n), rng.integers(0, n_windows, n)
    rows["class_index"] = rng.integers(0, n_classes, n)
    rows["confidence"] = rng.random(n, np.float32)
    rows = rows[np.lexsort((rows["window"], rows["recording"]))]
    veto = np.zeros(n_classes, np.uint8)
    veto[0] = 1
    flt = host.EventTables(np.full(n_classes, 0.5, np.float32), veto, 0.5, 30, 2, host.EVENTS_KEEP_DROPPED)
    got = host.detection_events(rows, n_classes, flt)                    # warm-up
    want, host_ms = timed(lambda: evref.events(rows, flt))
    same = bool(np.array_equal(got, want))
    ts = [timed(lambda: host.detection_events(rows, n_classes, flt))[1] for _ in range(rounds)]
    r = {"rows": n, "recordings": n_rec, "classes": n_classes, "events": int(got.size), "a_equals_b": same, "host_rule_once_ms": round(host_ms, 1),
         "device_tail_with_copies": stats(ts)}
    return r, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--overlaps", default="0,2.5")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--burst", type=int, default=400, help="recordings of 9 s in the burst (overlap 2.0 s), cut from the recording")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--floor-only", action="store_true")
    a = ap.parse_args()
    host.init()                                                          # no device: a loud error, not a fallback
    blob = sm.build_model(sm.SynthConfig())
    c = host.HipClassifier(blob, max_batch=a.max_batch)
    parent = None
    if a.parent_lib:
        mine = host._lib
        host._lib = host.load_library(a.parent_lib)                      # the second handle lives in the parent's library
        parent = host.HipClassifier(blob, max_batch=a.max_batch)
        host._lib = mine
    pcm = recording(a.seconds)
    res = {"tool": "analyze_events_rate", "seconds": a.seconds, "rate": RATE, "bits": 16, "max_batch": a.max_batch, "rounds": a.rounds, "k": a.k,
           "parent_lib": bool(a.parent_lib), "floor_only": a.floor_only, "overlaps": {}}
    ok = True
    for ov in [float(v) for v in a.overlaps.split(",")]:
        _, clip_len, hop, min_tail = wav.window_table([pcm.size], RATE, 3.0, ov)
        assert clip_len == CLIP
        r, same = legs(c, parent, pcm, [pcm.size], hop, min_tail, a.k, ov, a.rounds, a.floor_only)
        ok = ok and same
        res["overlaps"][str(ov)] = r
        print(json.dumps({str(ov): r}), file=sys.stderr, flush=True)
    if a.burst:
        n = 9 * RATE
        raw = pcm[:min(pcm.size, a.burst * n) // n * n]
        _, _, hop, min_tail = wav.window_table([n], RATE, 3.0, 2.0)
        r, same = legs(c, parent, raw, [n] * (raw.size // n), hop, min_tail, a.k, 2.0, a.rounds, a.floor_only)
        ok = ok and same
        res["burst_9s_overlap_2.0"] = r
        print(json.dumps({"burst": r}), file=sys.stderr, flush=True)
    if not a.floor_only:
        r, same = tail_alone(a.rounds)
        ok = ok and same
        res["tail_alone"] = r
    c.close()
    if parent is not None:
        parent.close()
    res["a_equals_b"] = ok
    print(json.dumps(res))
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
