"""File analysis of a directory of recordings at their own sample rates, on the full synthetic model, three ways (DESIGN section 9
"File analysis", mixed rates): eight 10-minute int16 recordings - two at 48 kHz and one each at 32, 44.1, 96, 192, 250 and 384 kHz -
  (a) one bnhip_analyze_mixed_pcm_topk call: every recording goes to the device once, as it is in its file, and is resampled,
      converted and framed there;
  (b) the path wav.analyze_files takes without device_resample: numpy conversion to float32, one bnhip_resample_f32 call per file
      that is not at the model's rate (float32 up, float32 down), then bnhip_analyze_pcm_topk(bits = 0) over the float32 recordings
      (up again).  Reported with and without the numpy conversion;
  (c) the floor: the same total audio already at 48 kHz int16 through bnhip_analyze_pcm_topk.
The legs run in one process, alternated round by round, host clock around calls that end in a synchronise; medians over --rounds
after one warm-up of each, every round's time kept (the spread).  (a) must equal (b) bit for bit: the tool's one hard assertion.
The bytes each leg moves over PCIe are counted from the shapes.  The library is the one host.py loads: BNHIP_LIB names another
build, so `--legs bc` against the parent commit's library gives (b) and (c) as they were before this entry existed.
Prints one JSON line and, with --out, writes it there.

    python tools/analyze_mixed_rate.py [--minutes 10] [--overlaps 0,2.0] [--rounds 3] [--max-batch 256] [--legs abc] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import birdnet_go_amd  # noqa: E402,F401
from birdnet_go_amd import host, synth_model as sm, wav  # noqa: E402

MODEL_RATE, CLIP = 48000, 144000
RATES = [48000, 48000, 32000, 44100, 96000, 192000, 250000, 384000]


def recording(rate, seconds, seed):
    """int16 material at `rate`: a minute of tones and noise, repeated with a level of its own per minute."""
    rng = np.random.default_rng(seed)
    n = 60 * rate
    t = np.arange(n, dtype=np.float32) / np.float32(rate)
    minute = np.zeros(n, np.float32)
    for f in (440.0 + 35.0 * seed, 2100.0 + 90.0 * seed, 6300.0):
        minute += np.sin(np.float32(2 * np.pi * f) * t)
    minute = minute / 3.2 + 0.05 * rng.standard_normal(n).astype(np.float32)
    reps = (seconds + 59) // 60
    out = np.empty(reps * n, np.int16)
    for i, level in enumerate(np.linspace(0.3, 0.9, reps)):
        out[i * n:(i + 1) * n] = np.round(minute * np.float32(level * 30000.0)).clip(-32768, 32767).astype(np.int16)
    return out[:seconds * rate]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=int, default=10)
    ap.add_argument("--overlaps", default="0,2.0")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--out", default="")        # (profiles/r23_analyze_mixed_rate.json collects several runs of this tool)
    a = ap.parse_args()
    host.init()                                                      # no device: a loud error, not a fallback
    seconds = a.minutes * 60
    pcm = [recording(rate, seconds, i) for i, rate in enumerate(RATES)]
    recs = host.recordings([x.size for x in pcm], RATES, 16)
    raw = np.concatenate([x.view(np.uint8) for x in pcm])
    floor = np.concatenate([recording(MODEL_RATE, seconds, 20 + i) for i in range(len(RATES))])
    resamplers = {rate: host.Resampler(rate, MODEL_RATE) for rate in set(RATES) if rate != MODEL_RATE}
    n_out = [x.size if rate == MODEL_RATE else resamplers[rate].estimate_output(x.size) for x, rate in zip(pcm, RATES)]
    c = host.HipClassifier(sm.build_model(sm.SynthConfig()), max_batch=a.max_batch)
    with open(host.LIB_PATH, "rb") as fh:
        digest = hashlib.sha256(fh.read()).hexdigest()[:16]
    n_in = [int(x.size) for x in pcm]
    res = {"tool": "analyze_mixed_rate", "library": os.path.relpath(host.LIB_PATH, ROOT), "library_sha256_16": digest, "legs": a.legs,
           "minutes": a.minutes, "rates": RATES, "model_rate": MODEL_RATE, "bits": 16, "max_batch": a.max_batch, "rounds": a.rounds,
           "samples_in": n_in, "samples_at_model_rate": [int(n) for n in n_out],
           # counted from the shapes: (a) the files' bytes; (b) float32 up and float32 down per resampled file, then every float32
           # recording up; (c) int16 at the model's rate
           "pcie_bytes": {"a": int(2 * sum(n_in)),
                          "b": int(sum(4 * n + 4 * m for n, m, r in zip(n_in, n_out, RATES) if r != MODEL_RATE) + 4 * sum(n_out)),
                          "c": int(2 * floor.size)},
           "overlaps": {}}
    ok = True
    for ov in [float(v) for v in a.overlaps.split(",")]:
        _, clip_len, hop, min_tail = wav.window_table([CLIP], MODEL_RATE, 3.0, ov)
        assert clip_len == CLIP
        t_conv = []

        def leg_a():
            return c.analyze_mixed_pcm_topk(raw, recs, MODEL_RATE, hop, min_tail, k=a.k)[:2]

        def leg_b():
            t0 = time.perf_counter()
            fl = [x.astype(np.float32) / np.float32(32768.0) for x in pcm]                 # wav.read_wav's conversion
            t_conv.append((time.perf_counter() - t0) * 1e3)
            fl = [s if rate == MODEL_RATE else resamplers[rate].resample_f32(s) for s, rate in zip(fl, RATES)]
            return c.analyze_pcm_topk(np.concatenate(fl), 0, [s.size for s in fl], hop, min_tail, k=a.k)[:2]

        def leg_c():
            return c.analyze_pcm_topk(floor, 16, [seconds * MODEL_RATE] * len(RATES), hop, min_tail, k=a.k)[:2]

        legs = [(n, f) for n, f in (("a", leg_a), ("b", leg_b), ("c", leg_c)) if n in a.legs]
        first = {n: f() for n, f in legs}                                # warm-up of every leg, and the comparison
        same = None
        if "a" in first and "b" in first:
            same = bool(np.array_equal(first["a"][0], first["b"][0]) and np.array_equal(first["a"][1], first["b"][1]))
            ok = ok and same
        t_conv.clear()
        ts = {n: [] for n, _ in legs}
        for _ in range(a.rounds):
            for n, f in legs:
                t0 = time.perf_counter()
                f()
                ts[n].append((time.perf_counter() - t0) * 1e3)
        w = int(next(iter(first.values()))[0].shape[0])
        r = {"hop": hop, "windows": w, "bit_identical_a_b": same}
        for n in ts:
            r[n + "_ms"] = round(float(np.median(ts[n])), 1)
            r[n + "_all_ms"] = [round(t, 1) for t in ts[n]]
            r[n + "_spread_ms"] = round(max(ts[n]) - min(ts[n]), 1)
        if "b" in ts:
            r["b_numpy_conversion_ms"] = round(float(np.median(t_conv)), 1)
            r["b_without_conversion_ms"] = round(float(np.median([t - v for t, v in zip(ts["b"], t_conv)])), 1)
        if "a" in ts and "b" in ts:
            r["speedup_a_over_b"] = round(r["b_ms"] / r["a_ms"], 2)
            r["speedup_a_over_b_without_conversion"] = round(r["b_without_conversion_ms"] / r["a_ms"], 2)
        if "a" in ts and "c" in ts:
            r["a_over_floor_c"] = round(r["a_ms"] / r["c_ms"], 2)
        res["overlaps"][str(ov)] = r
        print(json.dumps({str(ov): r}), file=sys.stderr, flush=True)
    c.close()
    res["bit_identical"] = ok
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
