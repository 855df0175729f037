"""One tick of the real-time path at 256 sources on the full synthetic model, answered as detection events (DESIGN section 9
"Real-time detection events"), measured these ways:
  parent_topk        bnhip_windows_predict_topk of a library built from the parent commit (--parent-lib), where there is one;
  topk               the same entry of this library;
  topk_host_rule     that entry, then the streaming rule on the host in Python (tests/evbankref.py, the restatement the tests pin to);
  topk_bank_process  that entry, then bnhip_event_bank_process on the rows it returned;
  fused_events       bnhip_windows_predict_events: the rows stay on the device and the bank runs behind the last chunk.
Every leg has an assembler of its own, fed the same bytes before each tick (not timed); the legs of a process (--legs) alternate
tick by tick, host clock around calls that end in a synchronise; p50 / p95 / min over --ticks after two warm-up rounds.  Two
libraries in one process, or many legs with their banks, share the process' few hardware queues and slow each other down
(profiles/r28_event_bank_rate.json, "one_process"), so the comparison that counts runs a leg per process - the parent's library
through BNHIP_LIB with --legs topk - and alternates the processes from outside.  The spread of a
leg against itself is the difference between the two halves of its own ticks ("self_spread_ms": p50 of the odd ticks minus p50 of
the even ones).  Every tick the fused events must equal the bank fed the returned rows, and both the restatement: asserted.  The
thresholds come from the warm-up rows: the median confidence for every class, the most frequent class as the veto class.  The
bytes the bank moves per tick are counted from the call's layout.  --bank-only N runs N bnhip_event_bank_process calls and nothing
else beside the one warm-up tick that makes their rows: the process for `rocprofv3 --kernel-trace`, whose k_evb_* rows are the bank's
kernel time.  Prints one JSON line.

    python tools/event_bank_rate.py [--ticks 40] [--sources 256] [--hold 10] [--legs a,b] [--parent-lib PATH] [--bank-only N]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import birdnet_go_amd  # noqa: E402,F401
from birdnet_go_amd import host, stream, synth_model as sm  # noqa: E402
import evbankref  # noqa: E402


def stats(ts):
    ts = np.asarray(ts)
    return {"p50_ms": round(float(np.percentile(ts, 50)), 3), "p95_ms": round(float(np.percentile(ts, 95)), 3), "min_ms": round(float(ts.min()), 3),
            "self_spread_ms": round(float(np.percentile(ts[1::2], 50) - np.percentile(ts[0::2], 50)), 3)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


class Leg:
    """An assembler of its own in `lib`, with the sources added."""

    def __init__(self, lib, n_src, ovb, rdb, clip_b):
        mine = host._lib
        host._lib = lib
        stream.NativeWindows._proto_done = False                         # the prototypes are set on this library's entries too
        try:
            self.win = stream.NativeWindows(ovb, rdb, 256)
        finally:
            host._lib = mine
        self.ids = [self.win.add_source(f"src{i}", 2 * clip_b) for i in range(n_src)]

    def write(self, fresh):
        for i in self.ids:
            self.win.write(i, fresh[i])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--sources", type=int, default=256)
    ap.add_argument("--hold", type=int, default=10, help="hold_windows: 15 s at the 1.5 s hop of these rings")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--bank-only", type=int, default=0)
    ap.add_argument("--legs", default="topk,topk_host_rule,topk_bank_process,fused_events")
    a = ap.parse_args()
    host.init()                                                          # no device: a loud error, not a fallback
    blob = sm.build_model(sm.SynthConfig())
    lib = host.load_library()
    clf = host.HipClassifier(blob, max_batch=256)
    n_src, k = a.sources, min(a.k, clf.num_species())
    nc = clf.num_species()
    clip_b = clf.n_samples * 2
    ovb, rdb = clip_b // 2, clip_b - clip_b // 2
    rng = np.random.default_rng(27)
    t = np.arange(rdb // 2) / 48000.0
    tones = np.stack([0.3 * np.sin(2 * np.pi * (500 + 37 * i) * t) for i in range(n_src)])

    def fresh_bytes():
        x = tones + rng.normal(0, 0.05, tones.shape)
        return (np.clip(x, -1, 1) * 32767).astype("<i2").view(np.uint8).reshape(n_src, -1)

    parent = parent_clf = None
    if a.parent_lib and not a.bank_only:
        plib = host.load_library(a.parent_lib)
        mine = host._lib
        host._lib = plib
        parent_clf = host.HipClassifier(blob, max_batch=256)            # the handle lives in the parent's library
        host._lib = mine
        parent = Leg(plib, n_src, ovb, rdb, clip_b)
    names = a.legs.split(",")
    legs = {n: Leg(lib, n_src, ovb, rdb, clip_b) for n in names}

    # warm-up tick: the rows the filter is made from
    fresh = fresh_bytes()
    warm = Leg(lib, n_src, ovb, rdb, clip_b)
    warm.write(fresh)
    idxs, _, conf, idx = warm.win.predict_topk(clf, 16, k, 0, 1.0)
    warm.win.close()
    assert idxs == list(range(n_src))
    thr = np.full(nc, np.float32(np.median(conf)), np.float32)
    veto = np.zeros(nc, np.uint8)
    heard = int(np.bincount(idx.reshape(-1), minlength=nc).argmax())
    veto[heard] = 1
    flt = host.EventTables(thr, veto, float(np.quantile(conf[idx == heard], 0.9)), a.hold, 2, host.EVENTS_KEEP_DROPPED)
    banks = {n: host.EventBank(nc, k, flt, n_src) for n in ("topk_bank_process", "fused_events") if n in names or a.bank_only}
    ref = evbankref.EventBank(n_src, nc, k, flt)
    res = {"tool": "event_bank_rate", "library": os.path.basename(host.LIB_PATH), "legs": names, "sources": n_src, "k": k, "n_classes": nc,
           "hold_windows": a.hold, "min_count": 2, "ticks": a.ticks, "slots_per_source": ref.slots_per_source, "parent_lib": bool(parent)}

    if a.bank_only:
        b = banks["topk_bank_process"]
        ts = [timed(lambda: b.process(idxs, conf, idx))[1] for _ in range(a.bank_only)]
        res["bank_process_alone"] = stats(ts)
        print(json.dumps(res))
        return

    ts = {n: [] for n in names + (["parent_topk"] if parent else [])}
    n_events, same = 0, True
    for tick in range(a.ticks + 2):
        fresh = fresh_bytes()
        for leg in list(legs.values()) + ([parent] if parent else []):
            leg.write(fresh)
        got = {}
        order = list(ts)
        order = order[tick % len(order):] + order[:tick % len(order)]    # no leg always runs behind the same one
        for n in order:
            w = (parent if n == "parent_topk" else legs[n]).win
            if n == "parent_topk":
                _, ms = timed(lambda: w.predict_topk(parent_clf, 16, k, 0, 1.0))
            elif n == "topk":
                _, ms = timed(lambda: w.predict_topk(clf, 16, k, 0, 1.0))
            elif n == "topk_host_rule":
                def f():
                    s, _, c, i = w.predict_topk(clf, 16, k, 0, 1.0)
                    return ref.process(s, c, i)
                got[n], ms = timed(f)
            elif n == "topk_bank_process":
                def f():
                    s, _, c, i = w.predict_topk(clf, 16, k, 0, 1.0)
                    return banks[n].process(s, c, i)
                got[n], ms = timed(f)
            else:
                out, ms = timed(lambda: clf.predict_windows_events(w, banks[n], 16, k, 0, 1.0))
                got[n] = out[4]
            if tick >= 2:
                ts[n].append(ms)
        answers = list(got.values())
        same = same and all(np.array_equal(answers[0], g) for g in answers[1:])
        n_events += int(answers[0].size) if answers else 0
    assert same, "the fused tick, the bank fed the rows and the restatement disagree"
    res.update({n: stats(v) for n, v in ts.items()})
    res["events_equal_every_tick"] = bool(same) if len(got) > 1 else None
    res["events_per_tick"] = round(n_events / (a.ticks + 2), 1)
    # what a bank call moves: the header up (32 bytes per source of the call, 4 per row), the count and the first events down; the host
    # form also takes the rows up; the filter's tables go up once per set_filter, not per tick
    per_tick_events = 32 * min(127, int(np.ceil(n_events / (a.ticks + 2))))
    res["bank_bytes_per_tick"] = {"fused_up": 32 * n_src + 4 * n_src, "fused_down": 16 + 32 * 127, "fused_down_used": 16 + per_tick_events,
                                  "host_form_rows_up": 8 * n_src * k, "rows_kept_on_device_d2d": 8 * n_src * k,
                                  "filter_tables_once": 5 * nc}
    if "fused_events" in res and "topk" in res:
        res["fused_minus_topk_p50_ms"] = round(res["fused_events"]["p50_ms"] - res["topk"]["p50_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
