"""Per-tick cost of feeding a 32 kHz model's rings from 48 kHz sources, two ways:
  (a) one StreamResampler per source (its own HIP stream, one blocking round trip per frame), then NativeWindows.write;
  (b) one bnhip_windows_write_resampled per tick (host.ResamplerBank: one H2D, one launch, one D2H, one synchronise).
256 sources, ~100 ms frames, 5 warm-up + 50 timed ticks per leg, host clock around work that ends in a synchronise (every call
of both legs returns only after its device work).  The legs alternate, twice each, in one process; after every leg the rings of
both assemblers are collected and compared byte for byte.  Prints one JSON line.

    python tools/resample_bank_rate.py [--sources 256] [--from 48000] [--to 32000] [--ticks 50] [--warmup 5]
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
    ap.add_argument("--from", dest="fr", type=int, default=48000)
    ap.add_argument("--to", type=int, default=32000)
    ap.add_argument("--ticks", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    host.init()                                                      # no device: a loud error, not a fallback
    n, frame = a.sources, a.fr // 10
    spec = S.ModelSpec(a.to, 5.0)                                    # Perch geometry at the target rate
    clip, overlap, read = spec.buffer_dimensions()
    total_ticks = a.rounds * (a.warmup + a.ticks)
    rng = np.random.default_rng(1)
    # one frame's worth per source per tick, drawn once; both legs consume the same frames in the same order
    frames = rng.integers(-20000, 20000, (total_ticks, n, frame), dtype=np.int16)
    wa, wb = S.NativeWindows(overlap, read, max_batch=n), S.NativeWindows(overlap, read, max_batch=n)
    sa = [wa.add_source(f"s{i}", 2 * clip) for i in range(n)]
    sb = [wb.add_source(f"s{i}", 2 * clip) for i in range(n)]
    rs = [host.StreamResampler(a.fr, a.to) for _ in range(n)]
    bank = host.ResamplerBank(a.fr, a.to, max_streams=n)
    st = [bank.add_stream() for _ in range(n)]
    fb = [[frames[t, i].tobytes() for i in range(n)] for t in range(total_ticks)]
    del frames

    def leg_a(t):
        for i in range(n):
            wa.write(sa[i], rs[i].resample_into(fb[t][i]))

    def leg_b(t):
        bank.write_windows(wb, [(st[i], sb[i], fb[t][i]) for i in range(n)])

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
    res = {"tool": "resample_bank_rate", "sources": n, "rate_in": a.fr, "rate_out": a.to, "frame_samples": frame,
           "timed_ticks_per_leg": len(times["a_per_source"]),
           "in_bytes_per_tick": n * frame * 2, "out_bytes_per_tick": n * (frame * a.to // a.fr) * 2}
    for name, v in times.items():
        res[f"{name}_p50_ms"] = round(pct(v, 50), 3)
        res[f"{name}_p95_ms"] = round(pct(v, 95), 3)
    res["speedup_p50"] = round(res["a_per_source_p50_ms"] / res["b_bank_p50_ms"], 2)
    res["rings_identical"] = bool(identical) and all(identical)
    res["checks"] = len(identical)
    print(json.dumps(res))
    for r in rs:
        r.close()
    bank.close()
    wa.close()
    wb.close()
    if not res["rings_identical"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
