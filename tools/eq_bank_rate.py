"""Per-tick cost of the analysis route's EQ + gain (AudioRouter.applyProcessing) on 256 sources, two ways:
  (a) one host.EqualizerBank call per source per frame (one blocking round trip each), then NativeWindows.write;
  (b) one bnhip_windows_write_equalized per tick (one H2D, one k_eq_bank launch, one D2H, one synchronise for every source).
Every source has the stock chain (HighPass 100 Hz + LowPass 15 kHz, Q 0.7, 1 pass each) and +6 dB gain; 100 ms frames at
48 kHz; 5 warm-up + 50 timed ticks per leg, host clock around work that ends in a synchronise.  The legs alternate, twice each,
in one process, each with its own bank; after every leg the rings of both assemblers are collected and compared byte for
byte.  Prints one JSON line.

    python tools/eq_bank_rate.py [--sources 256] [--rate 48000] [--gain-db 6] [--ticks 50] [--warmup 5]
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
from birdnet_go_amd import host  # noqa: E402
from birdnet_go_amd import stream as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=256)
    ap.add_argument("--rate", dest="fr", type=int, default=48000)
    ap.add_argument("--gain-db", type=float, default=6.0)
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    host.init()                                                      # no device: a loud error, not a fallback
    n, frame = a.sources, a.fr // 10
    spec = S.ModelSpec(a.fr, 3.0)                                    # BirdNET geometry at the source rate
    clip, overlap, read = spec.buffer_dimensions()
    total_ticks = a.rounds * (a.warmup + a.ticks)
    rng = np.random.default_rng(1)
    # one frame's worth per source per tick, drawn once; both legs consume the same frames in the same order
    frames = rng.integers(-20000, 20000, (total_ticks, n, frame), dtype=np.int16)
    wa, wb = S.NativeWindows(overlap, read, max_batch=n), S.NativeWindows(overlap, read, max_batch=n)
    sa = [wa.add_source(f"s{i}", 2 * clip) for i in range(n)]
    sb = [wb.add_source(f"s{i}", 2 * clip) for i in range(n)]
    chain = host.build_filter_chain({"enabled": True, "filters": [{"type": "HighPass", "frequency": 100, "q": 0.7},
                                                                  {"type": "LowPass", "frequency": 15000, "q": 0.7}]}, a.fr)
    banks = [host.EqualizerBank(max_streams=n) for _ in range(2)]
    st = [[bk.add_stream() for _ in range(n)] for bk in banks]
    for bk, ss in zip(banks, st):
        for s in ss:
            bk.set_chain(s, chain, host.gain_linear(a.gain_db))
    fb = [[frames[t, i].tobytes() for i in range(n)] for t in range(total_ticks)]
    del frames

    def leg_a(t):
        for i in range(n):
            wa.write(sa[i], banks[0].process([(st[0][i], fb[t][i])])[0])

    def leg_b(t):
        banks[1].write_windows(wb, [(st[1][i], sb[i], fb[t][i]) for i in range(n)])

    times = {"a_per_source": [], "b_bank": []}
    cursor = {"a_per_source": 0, "b_bank": 0}
    identical = []
    for _ in range(a.rounds):
        for name, fn in (("a_per_source", leg_a), ("b_bank", leg_b)):
            for k in range(a.warmup + a.ticks):
                t = cursor[name]
                cursor[name] += 1
                t0 = time.perf_counter()
                fn(t)
                dt = time.perf_counter() - t0
                if k >= a.warmup:
                    times[name].append(dt * 1e3)
            # after each leg: the rings that both legs have filled to the same point are compared
            if cursor["a_per_source"] == cursor["b_bank"]:
                ia, ra = wa.collect()
                ib, rb = wb.collect()
                identical.append(bool(ia == ib and np.array_equal(ra, rb)) and
                                 all(wa.stats(sa[i]) == wb.stats(sb[i]) for i in range(n)))
    pct = lambda v, q: float(np.percentile(np.asarray(v), q))
    res = {"tool": "eq_bank_rate", "sources": n, "rate": a.fr, "frame_samples": frame, "stages": sum(p for _, p in chain),
           "gain_db": a.gain_db, "timed_ticks_per_leg": len(times["a_per_source"]), "bytes_per_tick": n * frame * 2}
    for name, v in times.items():
        res[f"{name}_p50_ms"] = round(pct(v, 50), 3)
        res[f"{name}_p95_ms"] = round(pct(v, 95), 3)
    res["speedup_p50"] = round(res["a_per_source_p50_ms"] / res["b_bank_p50_ms"], 2)
    res["rings_identical"] = bool(identical) and all(identical)
    res["checks"] = len(identical)
    print(json.dumps(res))
    for bk in banks:
        bk.close()
    wa.close()
    wb.close()
    if not res["rings_identical"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
