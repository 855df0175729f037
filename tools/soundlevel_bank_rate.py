"""Per-tick cost of the 1/3-octave sound level monitor (soundlevel.Processor behind a SoundLevelConsumer per source) on 256
sources, three ways:
  (a) one host.SoundLevelBank call per source per frame (one blocking round trip each);
  (b) one host.SoundLevelBank call per tick for every source (one H2D, one k_soundlevel_bank launch, one D2H, one synchronise);
  (c) a single-thread CPU restatement of the same arithmetic: tests/native/soundlevel_ref.c (the band filters and block sums,
      built here with -O2 -ffp-contract=off) with tests/slref.py's schedule, dB and interval statistics.  A C and Python
      restatement, not the reference's Go.
Every source gets random PCM16 at 48 kHz in 100 ms frames, interval 1; 5 warm-up + 50 timed ticks per leg, host clock around
work that ends in a synchronise (or the CPU leg's return).  The legs alternate, twice each, in one process, each with its own
bank; each leg consumes the same frames in the same order, and the reports of every tick are compared across the legs.  Prints
one JSON line.

    python tools/soundlevel_bank_rate.py [--sources 256] [--rate 48000] [--ticks 50] [--warmup 5] [--rounds 2] [--legs abc]
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
from birdnet_go_amd import host  # noqa: E402
import slref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=256)
    ap.add_argument("--rate", dest="fr", type=int, default=48000)
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--legs", default="abc")
    a = ap.parse_args()
    host.init()                                                      # no device: a loud error, not a fallback
    n, frame = a.sources, a.fr // 10

    def frames(t):                                                   # tick t's frames, the same for every leg
        return np.random.default_rng(1000 + t).integers(-32768, 32768, (n, frame), dtype=np.int16)

    banks = {leg: host.SoundLevelBank(a.fr, max_streams=n) for leg in "ab" if leg in a.legs}
    st = {leg: [bk.add_stream(1) for _ in range(n)] for leg, bk in banks.items()}
    procs = {i: slref.Processor(a.fr, 1) for i in range(n)}
    slref._native_lib()                                              # built before anything is timed

    def norm(reps, src_of):
        return [(src_of(r), r["duration_seconds"], r["octave_bands"]) for r in reps]

    def leg_a(x):
        out = []
        for i in range(n):
            out += norm(banks["a"].process([(st["a"][i], x[i])]), lambda r, i=i: i)
        return out

    def leg_b(x):
        return norm(banks["b"].process([(st["b"][i], x[i]) for i in range(n)]), lambda r: r["frame"])

    def leg_c(x):
        return norm(slref.process(procs, [(i, x[i]) for i in range(n)], native=True), lambda r: r["stream"])

    legs = [(k, fn) for k, fn in (("a", leg_a), ("b", leg_b), ("c", leg_c)) if k in a.legs]
    names = {"a": "a_per_source", "b": "b_bank", "c": "c_cpu_restatement"}
    times = {k: [] for k, _ in legs}
    reports = {k: [] for k, _ in legs}
    cursor = {k: 0 for k, _ in legs}
    for _ in range(a.rounds):
        for k, fn in legs:
            for j in range(a.warmup + a.ticks):
                x = frames(cursor[k])
                cursor[k] += 1
                t0 = time.perf_counter()
                r = fn(x)
                dt = time.perf_counter() - t0
                reports[k].append(r)
                if j >= a.warmup:
                    times[k].append(dt * 1e3)
    pct = lambda v, q: float(np.percentile(np.asarray(v), q))
    res = {"tool": "soundlevel_bank_rate", "sources": n, "rate": a.fr, "frame_samples": frame, "interval_s": 1,
           "bands": len(host.sound_level_bands(a.fr)), "timed_ticks_per_leg": a.rounds * a.ticks,
           "samples_per_tick": n * frame}
    for k, _ in legs:
        res[f"{names[k]}_p50_ms"] = round(pct(times[k], 50), 3)
        res[f"{names[k]}_p95_ms"] = round(pct(times[k], 95), 3)
    if "a" in times and "b" in times:
        res["speedup_b_over_a_p50"] = round(res["a_per_source_p50_ms"] / res["b_bank_p50_ms"], 2)
    if "c" in times and "b" in times:
        res["speedup_b_over_c_p50"] = round(res["c_cpu_restatement_p50_ms"] / res["b_bank_p50_ms"], 2)
    ref = legs[0][0]
    checks = [t for t in range(len(reports[ref]))]
    res["reports"] = sum(len(r) for r in reports[ref])
    res["ticks_compared"] = len(checks)
    for k, _ in legs[1:]:
        res[f"reports_identical_{ref}_{k}"] = all(reports[ref][t] == reports[k][t] for t in checks)
    print(json.dumps(res))
    for bk in banks.values():
        bk.close()
    if not all(v for key, v in res.items() if key.startswith("reports_identical")):
        sys.exit(1)


if __name__ == "__main__":
    main()
