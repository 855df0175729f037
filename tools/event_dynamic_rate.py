"""What dynamic thresholds cost ("Dynamic thresholds"), a process per leg, the processes alternated round by round:
  plain        one tick of the real-time path at 256 sources on the full synthetic model through bnhip_windows_predict_events with a
               bank created without a dynamic - the workload of tools/event_bank_rate.py - in this tree and, with --parent-tree (a
               checkout of the parent commit with its library built), in that one: the same tool file, the other tree's package;
  dynamic      the same tick with a bank created dynamic: every class learns, and the trigger is the median confidence of the
               warm-up tick, so classes learn during the run; bank time is the tick number, valid 8 ticks, cooldown 2; every tick's
               events, change records and, at the end, class state must equal the restatement's (tests/dynref.py): asserted, outside
               the timing;
  host_rule    bnhip_windows_predict_topk, then the restatement in Python on the rows it returned.
Host clock around calls that end in a synchronise; per process p50 / p95 / min over --ticks after two warm-up rounds; per leg the
p50 of every round, their median and their spread (largest minus smallest), and the bytes the bank's call copies up and down per
tick, counted from what each tick brought and answered (the first copy back is 4 080 bytes; a tick with more than 127 events - 111
in a dynamic bank - or more than 16 change records makes a second copy).  --kernel-stats NAME=CSV (repeatable) folds the k_ev*
rows of a rocprofv3 kernel_stats.csv, one per trace run, into the result under the kernels' full names.  --bank-only N
(with --leg plain or dynamic) runs N bnhip_event_bank_process calls on one tick's rows and nothing else, bank time stepping by one:
the process for a kernel trace of the bank's kernels.

    python tools/event_dynamic_rate.py [--rounds 3] [--ticks 40] [--parent-tree PATH] [--kernel-stats NAME=CSV ...] [--out FILE]
    python tools/event_dynamic_rate.py --leg NAME [--tree PATH] [--ticks 40] [--bank-only N]      (one leg, one JSON line)
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOLD, MIN_COUNT = 10, 2
VALID, COOLDOWN = 8, 2


def stats(ts):
    ts = np.asarray(ts)
    return {"p50_ms": round(float(np.percentile(ts, 50)), 3), "p95_ms": round(float(np.percentile(ts, 95)), 3), "min_ms": round(float(ts.min()), 3)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


FIRST_COPY, FIRST_EVENTS, FIRST_RECORDS = 4080, 127, 16   # the copy that brings the count down, and what rides in it (api_event_bank.cpp)


def bank_bytes(sources, events, records, dynamic):
    """-> bytes up (32 per source of the call, 4 per row), bytes down (the first copy, and the second where there is one) of one
    bank call that brought one row of each of `sources` and answered `events` events and `records` change records."""
    first = FIRST_EVENTS - (FIRST_RECORDS if dynamic else 0)
    second = 32 * max(0, events - first) + (32 * records if records > FIRST_RECORDS else 0)
    return 32 * len(set(sources)) + 4 * len(sources), FIRST_COPY + second, second > 0


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
    heard = int(np.bincount(idx.reshape(-1), minlength=nc).argmax())
    veto[heard] = 1
    flt = host.EventTables(thr, veto, float(np.quantile(conf[idx == heard], 0.9)), HOLD, MIN_COUNT, host.EVENTS_KEEP_DROPPED)
    dyn = ref = None
    if name != "plain":
        import dynref
        import evbankref
        dyn = host.EventDynamic(None, float(thr[0]), float(thr[0]) / 8, VALID, COOLDOWN)
        ref = dynref.DynamicBank(evbankref.EventBank(n_src, nc, k, flt), dyn)
    bank = None if name == "host_rule" else host.EventBank(nc, k, flt, n_src, **({"dynamic": dyn} if dyn is not None else {}))
    res = {"sources": n_src, "k": k, "n_classes": nc, "slots_per_source": bank.slots_per_source if bank else ref.inner.slots_per_source,
           "bytes_up_per_table_change": None if bank is None else nc * (6 if name == "dynamic" else 5)}
    if a.bank_only:
        ts = []
        for i in range(a.bank_only):
            if dyn is not None:
                bank.set_now(i)
            ts.append(timed(lambda: bank.process(idxs, conf, idx))[1])
        res["bank_process_alone"] = stats(ts)
        if dyn is not None:
            res["change_records"] = int(bank.threshold_changes().size)
        return res
    ts, n_events, n_changes, copies = [], 0, 0, []
    for tick in range(a.ticks + 2):
        fresh = fresh_bytes()
        for i in ids:
            win.write(i, fresh[i])
        if name == "host_rule":
            def f():
                s, _, c, i = win.predict_topk(clf, 16, k, 0, 1.0)
                ref.set_now(tick)
                return ref.process(s, c, i)
            ev, ms = timed(f)
            n_changes += int(ref.take_changes().size)
            copies.append((0, n_src * k * 8, False))                     # no bank: the top-k rows come down to the rule
        else:
            if dyn is not None:
                bank.set_now(tick)
            out, ms = timed(lambda: clf.predict_windows_events(win, bank, 16, k, 0, 1.0))
            ev = out[4]
            got = np.zeros(0)
            if ref is not None:
                ref.set_now(tick)
                assert np.array_equal(ev, ref.process(out[0], out[2], out[3])), "the dynamic bank's events and the restatement's differ"
                got = bank.threshold_changes()
                assert got.tobytes() == ref.take_changes().tobytes(), "the dynamic bank's change records and the restatement's differ"
                n_changes += int(got.size)
            copies.append(bank_bytes(out[0], int(ev.size), int(got.size), dyn is not None))
        n_events += int(ev.size)
        if tick >= 2:
            ts.append(ms)
    if bank is not None and ref is not None:
        assert all(g.tobytes() == w.tobytes() for g, w in zip(bank.thresholds(), ref.thresholds())), "the class state and the restatement's differ"
    res.update(stats(ts), events_per_tick=round(n_events / (a.ticks + 2), 1),
               bytes_up_per_tick=round(float(np.mean([c[0] for c in copies])), 1), bytes_down_per_tick=round(float(np.mean([c[1] for c in copies])), 1),
               bytes_down_first_copy=FIRST_COPY if bank is not None else None, ticks_with_second_copy=sum(c[2] for c in copies), ticks_counted=len(copies))
    if ref is not None:
        res.update(change_records=n_changes, classes_lowered_at_end=int((ref.thresholds()[0] > 0).sum()))
    return res


def one_leg(a):
    tree = os.path.abspath(a.tree) if a.tree else HERE
    sys.path.insert(0, tree)
    import birdnet_go_amd  # noqa: F401
    from birdnet_go_amd import host, stream, synth_model as sm
    host.init()                                                          # no device: a loud error, not a fallback
    res = {"tool": "event_dynamic_rate", "leg": a.leg, "tree": "parent" if a.tree else "this", "ticks": a.ticks}
    res.update(tick_leg(a, host, stream, sm, a.leg))
    print(json.dumps(res))


def drive(a):
    legs = [("plain", None), ("dynamic", None), ("host_rule", None)]
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
    out = {"tool": "event_dynamic_rate", "rounds": a.rounds, "ticks": a.ticks, "sources": a.sources, "hold_windows": HOLD, "min_count": MIN_COUNT,
           "valid": VALID, "cooldown": COOLDOWN, "legs": {}}
    for name, rs in runs.items():
        p50 = [x["p50_ms"] for x in rs]
        out["legs"][name] = {"p50_ms_by_round": p50, "p95_ms_by_round": [x["p95_ms"] for x in rs], "p50_ms": round(float(np.median(p50)), 3),
                             "spread_between_rounds_ms": round(max(p50) - min(p50), 3), "min_ms": min(x["min_ms"] for x in rs),
                             **{k: rs[-1][k] for k in ("slots_per_source", "events_per_tick", "change_records", "classes_lowered_at_end",
                                                       "bytes_up_per_tick", "bytes_down_per_tick", "bytes_down_first_copy", "ticks_with_second_copy",
                                                       "ticks_counted", "bytes_up_per_table_change") if k in rs[-1]}}
    for spec in a.kernel_stats or []:
        name, path = spec.split("=", 1)
        with open(path, newline="") as f:
            out.setdefault("kernel_trace", {})[name] = [
                {"kernel": r["Name"], "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(int(r["MinNs"]) / 1e3, 2),
                 "max_us": round(int(r["MaxNs"]) / 1e3, 2)} for r in csv.DictReader(f) if "k_ev" in r["Name"]]
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
    ap.add_argument("--kernel-stats", action="append", default=None, metavar="NAME=CSV")
    ap.add_argument("--leg", default=None, choices=["plain", "dynamic", "host_rule"])
    ap.add_argument("--tree", default=None)
    ap.add_argument("--bank-only", type=int, default=0)
    a = ap.parse_args()
    one_leg(a) if a.leg else drive(a)


if __name__ == "__main__":
    main()
