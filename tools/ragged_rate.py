"""Cost of a burst of detections of unequal lengths ("ragged bursts"): 64 clips at 48 kHz with 64 distinct lengths
between 9 s and 45 s (conf.ExtendedCaptureSettings: a detection is as long as the bird kept calling, to the sample), material from
tools/loudness_rate.py's generator, the export plan (-23 LUFS, -1 dBTP, +-60 dB, gate fallback), no seek table, lpc_order 8:
  (r) bnhip_loudness_flac_ragged_pcm16, the whole burst in one call;
  (p) flac.normalize_and_encode(ragged=False): the grouped path, one bnhip_loudness_flac_lpc_pcm16 call per distinct length - here
      one per clip;
  (b) and (d) of tools/flac_rate.py on its uniform burst (64 clips of 15 s): the fused call without LPC, and launch_flac alone on
      device-resident clips - the guards that show what the uniform path pays for the ragged geometry.
The library is the one host.py loads: BNHIP_LIB names another build, so the same tool run against the parent commit's library
(--legs pbd: it has no ragged entry) gives the baseline and the guards' other side.  Host clock around calls that end in a
synchronise; --warmup warm-up and --reps timed repetitions per leg, the legs alternated twice (half the repetitions per pass).
(r) is checked against (p) in every record and byte.  Prints one JSON line and writes it to --out.

    python tools/ragged_rate.py [--legs rpbd] [--reps 20] [--warmup 3] [--seed 16] [--out profiles/r16_ragged_rate.json]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import birdnet_go_amd  # noqa: E402,F401
from birdnet_go_amd import flac, host  # noqa: E402
from loudness_rate import PLAN, clips_48k, fields  # noqa: E402


def burst_lengths(n_clips, rate, seed, lo_s=9, hi_s=45):
    """n_clips distinct lengths in samples, uniform in [lo_s, hi_s] seconds, the shortest and the longest included."""
    rng = np.random.default_rng(seed)
    lens = rng.choice(np.arange(lo_s * rate + 1, hi_s * rate), n_clips - 2, replace=False).tolist()
    lens = [lo_s * rate] + lens + [hi_s * rate]
    return [int(lens[i]) for i in rng.permutation(n_clips)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="rpbd")
    ap.add_argument("--seed", type=int, default=16)
    ap.add_argument("--lpc-order", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_ragged_rate.json"))
    a = ap.parse_args()
    host.init()                                                      # no device: a loud error, not a fallback
    rate, M = 48000, a.lpc_order
    plan = (PLAN["target_lufs"], PLAN["true_peak_dbtp"], PLAN["max_gain_db"], PLAN["gate_fallback"])
    lens = burst_lengths(a.clips, rate, a.seed)
    long_clips = clips_48k(a.clips, 45, rate)
    burst = [np.ascontiguousarray(long_clips[i, :n]) for i, n in enumerate(lens)]
    uniform = np.ascontiguousarray(long_clips[:, :15 * rate])        # (flac_rate.py's burst: the generator's first 15 s are not its 15 s clips')
    del long_clips
    with open(host.LIB_PATH, "rb") as fh:
        digest = hashlib.sha256(fh.read()).hexdigest()[:16]
    res = {"tool": "ragged_rate", "library": os.path.relpath(host.LIB_PATH, ROOT), "library_sha256_16": digest, "clips": a.clips, "rate": rate,
           "seed": a.seed, "lengths": lens, "distinct_lengths": len(set(lens)), "pcm_bytes": int(2 * sum(lens)), "plan": PLAN,
           "seek_interval": 0, "lpc_order": M, "reps": a.reps, "warmup": a.warmup, "uniform_clips_seconds": [a.clips, 15]}
    kw = dict(max_gain_db=PLAN["max_gain_db"], gate_fallback=PLAN["gate_fallback"], lpc_order=M)
    legs = {"r": lambda: host.loudness_flac_ragged(burst, rate, *plan, lpc_order=M),
            "p": lambda: flac.normalize_and_encode(burst, rate, ragged=False, **kw),
            "b": lambda: host.loudness_flac(uniform, rate, *plan)}
    blocks = []
    if "d" in a.legs:
        # device memory through the HIP runtime the library itself uses
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipFree.argtypes = [C.c_void_p]

        def dev(nbytes):
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), nbytes) == 0
            blocks.append(p)
            return p
        B, n = uniform.shape
        _, gained = host.loudness_normalize(uniform, rate, *plan)
        cap, ws = host.flac_max_bytes(B, n, 0), host.flac_workspace_size(B, n)
        d_in, d_out, d_off, d_ws = dev(gained.nbytes), dev(cap), dev(8 * (B + 1)), dev(ws)
        assert hip.hipMemcpy(d_in, gained.ctypes.data, gained.nbytes, 1) == 0

        def leg_d():
            host.flac_encode_device(d_in, B, n, rate, d_out, cap, d_off, d_ws, ws)
            assert hip.hipDeviceSynchronize() == 0
        legs["d"] = leg_d
    run = [l for l in "rpbd" if l in a.legs]
    ts, got = {l: [] for l in run}, {}
    for l in run:
        for _ in range(a.warmup):
            legs[l]()
    for p in range(2):                                               # the legs alternated twice
        for l in run:
            for _ in range(a.reps // 2):
                t0 = time.perf_counter()
                got[l] = legs[l]()
                ts[l].append((time.perf_counter() - t0) * 1e3)
    names = {"r": "r_ragged_one_call", "p": "p_grouped_per_length", "b": "b_uniform_normalize_flac", "d": "d_uniform_flac_device_resident"}
    for l in run:
        v = np.array(ts[l])
        res[names[l] + "_ms"] = round(float(np.median(v)), 3)
        res[names[l] + "_min_ms"] = round(float(v.min()), 3)
        res[names[l] + "_pass_medians_ms"] = [round(float(np.median(h)), 3) for h in np.split(v, 2)]
    ok = True
    if "r" in run:
        r, streams = got["r"]
        res["compressed_bytes"] = sum(len(s) for s in streams)
        res["compression_ratio"] = round(res["compressed_bytes"] / res["pcm_bytes"], 4)
        res["r_clips_gate_lifted"] = sum(1 for g in r if g.flags & host.LOUDNESS_GATE_LIFTED)
    if "r" in run and "p" in run:
        res["r_equals_p"] = bool(fields(got["r"][0]) == fields(got["p"][0]) and got["r"][1] == got["p"][1])
        res["speedup_r_over_p"] = round(res["p_grouped_per_length_ms"] / res["r_ragged_one_call_ms"], 2)
        ok = ok and res["r_equals_p"]
    for p in blocks:
        hip.hipFree(p)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
