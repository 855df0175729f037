"""What extended capture costs ("Extended capture"), a process per leg, the processes alternated round by round:
  plain        one tick of the real-time path at 256 sources on the full synthetic model through bnhip_windows_predict_events with a
               bank created without an extend - the workload of tools/event_bank_rate.py - in this tree and, with --parent-tree (a
               checkout of the parent commit with its library built), in that one: the same tool file, the other tree's package;
  extended     the same tick with a bank created extended: waits 10 / 20 / 40 windows, max_windows 400, every class sliding; every
               tick's events must equal the streaming restatement's (tests/evxref.py): asserted, outside the timing;
  host_rule    bnhip_windows_predict_topk, then the restatement's streaming rule in Python on the rows it returned;
  tail_plain   bnhip_detection_events over the rows of an hour at overlap 2.5 s (7 195 windows, 71 950 rows), in both trees;
  tail         bnhip_detection_events_extended over the same rows; must equal the one-shot restatement: asserted.
Host clock around calls that end in a synchronise; per process p50 / p95 / min over --ticks after two warm-up rounds; per leg the
p50 of every round, their median and their spread (largest minus smallest).  --bank-only N (with --leg plain or extended) runs N
bnhip_event_bank_process calls on one tick's rows and nothing else: the process for a kernel trace of k_evb_update.

    python tools/event_extend_rate.py [--rounds 3] [--ticks 40] [--parent-tree PATH] [--out FILE]
    python tools/event_extend_rate.py --leg NAME [--tree PATH] [--ticks 40] [--bank-only N]      (one leg, one JSON line)
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAITS = dict(max_windows=400, short_wait=10, medium_from=20, medium_wait=20, long_from=80, long_wait=40)
HOLD, MIN_COUNT = 10, 2


def stats(ts):
    ts = np.asarray(ts)
    return {"p50_ms": round(float(np.percentile(ts, 50)), 3), "p95_ms": round(float(np.percentile(ts, 95)), 3), "min_ms": round(float(ts.min()), 3)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def hour_rows(host, nc, k=10, n_win=7195):
    """An hour's rows: three species that call in runs of up to 200 windows, the rest of each window's k results scattered."""
    rng = np.random.default_rng(30)
    rows = np.zeros(n_win * k, host.DETECTION)
    callers, left = rng.integers(0, nc, 3), np.zeros(3, np.int64)
    for w in range(n_win):
        for j in range(3):
            if left[j] <= 0:
                callers[j], left[j] = rng.integers(0, nc), rng.integers(1, 200)
            left[j] -= 1
        cls = np.concatenate([callers, rng.integers(0, nc, k - 3)])
        r = rows[w * k:(w + 1) * k]
        r["window"], r["class_index"], r["confidence"] = w, cls, (rng.integers(16, 64, k) / 64.0).astype(np.float32)
    return rows


def tail_leg(a, host, extended):
    sys.path.insert(0, os.path.join(HERE, "tests"))
    nc = 6522
    rows = hour_rows(host, nc)
    flt = host.EventTables(np.full(nc, 0.5, np.float32), None, 0.0, HOLD, MIN_COUNT, host.EVENTS_KEEP_DROPPED)
    kw = {}
    if extended:
        import evxref
        kw["extend"] = host.EventExtend(None, **WAITS)
        assert np.array_equal(host.detection_events(rows, nc, flt, **kw), evxref.events(rows, flt, kw["extend"]))
    ts, n = [], 0
    for i in range(a.ticks + 2):
        ev, ms = timed(lambda: host.detection_events(rows, nc, flt, **kw))
        n = int(ev.size)
        if i >= 2:
            ts.append(ms)
    return dict(stats(ts), rows=int(rows.size), events=n, longest_event=int((ev["last_window"] - ev["first_window"]).max()))


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

    def assembler():
        w = stream.NativeWindows(ovb, rdb, 256)
        return w, [w.add_source(f"src{i}", 2 * clip_b) for i in range(n_src)]

    win, ids = assembler()
    fresh = fresh_bytes()
    for i in ids:
        win.write(i, fresh[i])
    idxs, _, conf, idx = win.predict_topk(clf, 16, k, 0, 1.0)           # the warm-up tick: the rows the filter is made from
    thr = np.full(nc, np.float32(np.median(conf)), np.float32)
    veto = np.zeros(nc, np.uint8)
    heard = int(np.bincount(idx.reshape(-1), minlength=nc).argmax())
    veto[heard] = 1
    flt = host.EventTables(thr, veto, float(np.quantile(conf[idx == heard], 0.9)), HOLD, MIN_COUNT, host.EVENTS_KEEP_DROPPED)
    ext = ref = None
    if name != "plain":
        import evxref
        ext = host.EventExtend(None, **WAITS)
        ref = evxref.EventBank(n_src, nc, k, flt, ext)
    bank = None if name == "host_rule" else host.EventBank(nc, k, flt, n_src, **({"extend": ext} if ext is not None else {}))
    res = {"sources": n_src, "k": k, "n_classes": nc, "slots_per_source": bank.slots_per_source if bank else ref.slots_per_source}
    if a.bank_only:
        res["bank_process_alone"] = stats([timed(lambda: bank.process(idxs, conf, idx))[1] for _ in range(a.bank_only)])
        return res
    ts, n_events = [], 0
    for tick in range(a.ticks + 2):
        fresh = fresh_bytes()
        for i in ids:
            win.write(i, fresh[i])
        if name == "host_rule":
            def f():
                s, _, c, i = win.predict_topk(clf, 16, k, 0, 1.0)
                return ref.process(s, c, i)
            ev, ms = timed(f)
        else:
            out, ms = timed(lambda: clf.predict_windows_events(win, bank, 16, k, 0, 1.0))
            ev = out[4]
            if ref is not None:
                assert np.array_equal(ev, ref.process(out[0], out[2], out[3])), "the extended bank and the restatement disagree"
        n_events += int(ev.size)
        if tick >= 2:
            ts.append(ms)
    res.update(stats(ts), events_per_tick=round(n_events / (a.ticks + 2), 1))
    return res


def one_leg(a):
    tree = os.path.abspath(a.tree) if a.tree else HERE
    sys.path.insert(0, tree)
    import birdnet_go_amd  # noqa: F401
    from birdnet_go_amd import host, stream, synth_model as sm
    host.init()                                                          # no device: a loud error, not a fallback
    res = {"tool": "event_extend_rate", "leg": a.leg, "tree": "parent" if a.tree else "this", "ticks": a.ticks}
    if a.leg in ("tail", "tail_plain"):
        res.update(tail_leg(a, host, a.leg == "tail"))
    else:
        res.update(tick_leg(a, host, stream, sm, a.leg))
    print(json.dumps(res))


def drive(a):
    legs = [("plain", None), ("extended", None), ("host_rule", None), ("tail_plain", None), ("tail", None)]
    if a.parent_tree:
        legs[1:1] = [("plain", a.parent_tree)]
        legs.insert(-1, ("tail_plain", a.parent_tree))
    runs = {}
    for r in range(a.rounds):
        for leg, tree in legs[r % len(legs):] + legs[:r % len(legs)]:   # no leg always runs behind the same one
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--ticks", str(a.ticks), "--sources", str(a.sources)]
            p = subprocess.run(cmd + (["--tree", tree] if tree else []), capture_output=True, text=True, timeout=300)
            if p.returncode != 0:                                        # a leg that failed ends the run: nothing more is started
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit(p.returncode)
            runs.setdefault(leg + ("@parent" if tree else ""), []).append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(f"round {r}: {leg}{'@parent' if tree else ''} p50 {runs[leg + ('@parent' if tree else '')][-1]['p50_ms']} ms", file=sys.stderr, flush=True)
    out = {"tool": "event_extend_rate", "rounds": a.rounds, "ticks": a.ticks, "sources": a.sources, "hold_windows": HOLD, "min_count": MIN_COUNT,
           "extend": WAITS, "legs": {}}
    for name, rs in runs.items():
        p50 = [x["p50_ms"] for x in rs]
        out["legs"][name] = {"p50_ms_by_round": p50, "p50_ms": round(float(np.median(p50)), 3), "spread_between_rounds_ms": round(max(p50) - min(p50), 3),
                             "min_ms": min(x["min_ms"] for x in rs), "p95_ms": max(x["p95_ms"] for x in rs),
                             **{k: rs[-1][k] for k in ("slots_per_source", "events_per_tick", "rows", "events", "longest_event") if k in rs[-1]}}
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
    ap.add_argument("--leg", default=None, choices=["plain", "extended", "host_rule", "tail_plain", "tail"])
    ap.add_argument("--tree", default=None)
    ap.add_argument("--bank-only", type=int, default=0)
    a = ap.parse_args()
    one_leg(a) if a.leg else drive(a)


if __name__ == "__main__":
    main()
