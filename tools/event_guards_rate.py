"""What the dog-bark and daylight filters cost ("Dog-bark and daylight filters"), a process per leg, the processes
alternated round by round:
  plain        one tick of the real-time path at 256 sources on the full synthetic model through bnhip_windows_predict_events with a
               bank that never had guards set - the workload of tools/event_dynamic_rate.py's plain leg - in this tree and, with
               --parent-tree (a checkout of the parent commit with its library built), in that one: the same tool file, the other
               tree's package;
  guarded      the same tick with guards set on the bank: the class heard second most often is the dog class, a dog hit above the
               0.9 quantile of its warm-up confidences; the even classes are dropped by a bark at most hold_windows back, the
               classes 1 mod 4 in daylight, and every source has the daylight spans [4, 12) and [24, 34) of its own clock; every
               tick's events must equal the restatement's (tests/guardref.py): asserted, outside the timing; the share of events
               that the two guards drop is reported;
  host_rule    bnhip_windows_predict_topk, then the restatement in Python on the rows it returned: what a host does today.
Host clock around calls that end in a synchronise; per process p50 / p95 / min over --ticks after two warm-up rounds; per leg the
p50 of every round, their median and their spread (largest minus smallest), and the bytes the bank's call copies up per tick (32
per source and 4 per row; under guards with daylight spans 64 more per source).

    python tools/event_guards_rate.py [--rounds 3] [--ticks 40] [--parent-tree PATH] [--out FILE]
    python tools/event_guards_rate.py --leg NAME [--tree PATH] [--ticks 40]      (one leg, one JSON line)
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOLD, MIN_COUNT = 10, 2
SPANS = [(4, 12), (24, 34)]


def stats(ts):
    ts = np.asarray(ts)
    return {"p50_ms": round(float(np.percentile(ts, 50)), 3), "p95_ms": round(float(np.percentile(ts, 95)), 3), "min_ms": round(float(ts.min()), 3)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def tick_leg(a, host, stream, sm, name):
    sys.path.insert(0, os.path.join(HERE, "tests"))
    blob = sm.build_model(sm.SynthConfig())
    clf = host.HipClassifier(blob, max_batch=256)
    n_src, nc = a.sources, clf.num_species()
    k = min(10, nc)
    clip_b = clf.n_samples * 2
    ovb, rdb = clip_b // 2, clip_b - clip_b // 2
    rng = np.random.default_rng(27)
    t = np.arange(rdb // 2) / 48000.0
    tones = np.stack([0.3 * np.sin(2 * np.pi * (500 + 37 * i) * t) for i in range(n_src)])

    def fresh_bytes():
        x = tones + rng.normal(0, 0.05, tones.shape)
        return (np.clip(x, -1, 1) * 32767).astype("<i2").view(np.uint8).reshape(n_src, -1)

    win = stream.NativeWindows(ovb, rdb, 256)
    ids = [win.add_source(f"src{i}", 2 * clip_b) for i in range(n_src)]
    fresh = fresh_bytes()
    for i in ids:
        win.write(i, fresh[i])
    idxs, _, conf, idx = win.predict_topk(clf, 16, k, 0, 1.0)           # the warm-up tick: the rows the filter is made from
    thr = np.full(nc, np.float32(np.median(conf)), np.float32)
    veto = np.zeros(nc, np.uint8)
    order = np.argsort(-np.bincount(idx.reshape(-1), minlength=nc), kind="stable")
    heard, dog_class = int(order[0]), int(order[1])
    veto[heard] = 1
    flt = host.EventTables(thr, veto, float(np.quantile(conf[idx == heard], 0.9)), HOLD, MIN_COUNT, host.EVENTS_KEEP_DROPPED)
    guards = ref = None
    if name != "plain":
        import guardref
        dog = np.zeros(nc, np.uint8)
        dog[dog_class] = 1
        guards = host.EventGuards(dog, float(np.quantile(conf[idx == dog_class], 0.9)), (np.arange(nc) % 2 == 0).astype(np.uint8), HOLD,
                                  (np.arange(nc) % 4 == 1).astype(np.uint8))
        ref = guardref.EventBank(n_src, nc, k, flt, None, guards)
        for s in range(n_src):
            ref.set_daylight(s, SPANS)
    bank = None
    if name != "host_rule":
        bank = host.EventBank(nc, k, flt, n_src)
        if guards is not None:
            bank.set_guards(guards)
            for s in range(n_src):
                bank.set_daylight(s, SPANS)
    res = {"sources": n_src, "k": k, "n_classes": nc, "slots_per_source": bank.slots_per_source if bank else ref.slots_per_source}
    ts, status, up = [], np.zeros(5, np.int64), []
    for tick in range(a.ticks + 2):
        fresh = fresh_bytes()
        for i in ids:
            win.write(i, fresh[i])
        if name == "host_rule":
            def f():
                s, _, c, i = win.predict_topk(clf, 16, k, 0, 1.0)
                return ref.process(s, c, i)
            ev, ms = timed(f)
            up.append(0)
        else:
            out, ms = timed(lambda: clf.predict_windows_events(win, bank, 16, k, 0, 1.0))
            ev = out[4]
            if ref is not None:
                assert np.array_equal(ev, ref.process(out[0], out[2], out[3])), "the guarded bank's events and the restatement's differ"
            up.append((32 + (64 if guards is not None else 0)) * len(set(out[0])) + 4 * len(out[0]))
        status += np.bincount(ev["status"], minlength=5)[:5]
        if tick >= 2:
            ts.append(ms)
    n_events = int(status.sum())
    res.update(stats(ts), events_per_tick=round(n_events / (a.ticks + 2), 1), events_by_status=status.tolist(),
               share_dropped_by_guards=round(float(status[3] + status[4]) / max(n_events, 1), 4), bytes_up_per_tick=round(float(np.mean(up)), 1))
    return res


def one_leg(a):
    tree = os.path.abspath(a.tree) if a.tree else HERE
    sys.path.insert(0, tree)
    import birdnet_go_amd  # noqa: F401
    from birdnet_go_amd import host, stream, synth_model as sm
    host.init()                                                          # no device: a loud error, not a fallback
    res = {"tool": "event_guards_rate", "leg": a.leg, "tree": "parent" if a.tree else "this", "ticks": a.ticks}
    res.update(tick_leg(a, host, stream, sm, a.leg))
    print(json.dumps(res))


def drive(a):
    legs = [("plain", None), ("guarded", None), ("host_rule", None)]
    if a.parent_tree:
        legs[0:0] = [("plain", a.parent_tree)]
    runs = {}
    for r in range(a.rounds):
        for leg, tree in legs[r % len(legs):] + legs[:r % len(legs)]:   # no leg always runs behind the same one
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--ticks", str(a.ticks), "--sources", str(a.sources)]
            p = subprocess.run(cmd + (["--tree", tree] if tree else []), capture_output=True, text=True, timeout=300)
            if p.returncode != 0:                                        # a leg that failed ends the run: nothing more is started
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit(p.returncode)
            key = leg + ("@parent" if tree else "")
            runs.setdefault(key, []).append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(f"round {r}: {key} p50 {runs[key][-1]['p50_ms']} ms", file=sys.stderr, flush=True)
    out = {"tool": "event_guards_rate", "rounds": a.rounds, "ticks": a.ticks, "sources": a.sources, "hold_windows": HOLD, "min_count": MIN_COUNT,
           "dog_remember_windows": HOLD, "daylight_spans": SPANS, "legs": {}}
    for name, rs in runs.items():
        p50 = [x["p50_ms"] for x in rs]
        out["legs"][name] = {"p50_ms_by_round": p50, "p95_ms_by_round": [x["p95_ms"] for x in rs], "p50_ms": round(float(np.median(p50)), 3),
                             "spread_between_rounds_ms": round(max(p50) - min(p50), 3), "min_ms": min(x["min_ms"] for x in rs),
                             **{k: rs[-1][k] for k in ("slots_per_source", "events_per_tick", "events_by_status", "share_dropped_by_guards",
                                                       "bytes_up_per_tick") if k in rs[-1]}}
    text = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--sources", type=int, default=256)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, choices=["plain", "guarded", "host_rule"])
    ap.add_argument("--tree", default=None)
    a = ap.parse_args()
    one_leg(a) if a.leg else drive(a)


if __name__ == "__main__":
    main()
