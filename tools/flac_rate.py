"""Cost of encoding a burst of detections to FLAC on the device: 64 clips of 15 s at 48 kHz from
tools/loudness_rate.py's generator, the export plan (-23 LUFS, -1 dBTP, +-60 dB, gate fallback), no seek table:
  (a) bnhip_loudness_normalize_pcm16, one call: the baseline - the normalised PCM back on the host, not yet encoded;
  (b) bnhip_loudness_flac_pcm16, one call: loudness records, offsets and compressed bytes back on the host;
  (c) (b) as one call per clip;
  (d) bnhip_flac_encode_device on gained clips, output and workspace already on the device, synchronised: launch_flac's kernels
      alone (their per-kernel split comes from a kernel trace of this leg run on its own:
      rocprofv3 --kernel-trace --stats -- python tools/flac_rate.py --legs d, summarised by tools/prof_summary.py);
  (e) the bytes copied device-to-host in (a) and in (b), counted from the entries' contracts and checked against the offsets;
  (f) (b) with LPC predictors, lpc_order = --lpc-order (8: the reference's level), and (g) (d) likewise: the same burst, beside
      (b) and (d) in the same alternation; their compression and (e) of (f) are reported beside (b)'s.
Host clock around calls that end in a synchronise; --warmup warm-up and --reps timed repetitions per leg, the legs alternated
twice (half the repetitions per pass).  (b) is checked against (a) followed by bnhip_flac_encode_pcm16, (c) and (d) against (b),
byte for byte; clip 0 of (b) is decoded by tests/flacdec.py; (f) against (a) followed by the encode at that lpc_order, (g) against
(f), clip 0 of (f) decoded by tests/flaclpcdec.py.  Prints one JSON line and writes it to --out.

    python tools/flac_rate.py [--clips 64] [--seconds 15] [--reps 20] [--warmup 3] [--legs abcdfg] [--lpc-order 8]
                              [--out profiles/r15_flac_lpc_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import birdnet_go_amd  # noqa: E402,F401
from birdnet_go_amd import host  # noqa: E402
from loudness_rate import PLAN, clips_48k, fields  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="abcdfg")
    ap.add_argument("--lpc-order", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_flac_lpc_rate.json"))
    a = ap.parse_args()
    host.init()                                                      # no device: a loud error, not a fallback
    rate = 48000
    pcm = clips_48k(a.clips, a.seconds, rate)
    B, n = pcm.shape
    plan = (PLAN["target_lufs"], PLAN["true_peak_dbtp"], PLAN["max_gain_db"], PLAN["gate_fallback"])
    res = {"tool": "flac_rate", "clips": B, "seconds": a.seconds, "rate": rate, "plan": PLAN, "seek_interval": 0, "reps": a.reps,
           "warmup": a.warmup, "frames_per_clip": (n + 4095) // 4096, "pcm_bytes": int(pcm.nbytes), "lpc_order": a.lpc_order}
    M = a.lpc_order

    legs = {"a": lambda: host.loudness_normalize(pcm, rate, *plan),
            "b": lambda: host.loudness_flac(pcm, rate, *plan),
            "c": lambda: [host.loudness_flac(c, rate, *plan) for c in pcm],
            "f": lambda: host.loudness_flac(pcm, rate, *plan, lpc_order=M)}
    # the reference answers, once: (a), then the host-pointer encoder on its output
    want_res, gained = legs["a"]()
    want_streams = host.flac_encode(gained, rate)
    total = sum(len(s) for s in want_streams)
    want_lpc = host.flac_encode(gained, rate, lpc_order=M) if ("f" in a.legs or "g" in a.legs) else None
    if "d" in a.legs or "g" in a.legs:
        # device memory through the HIP runtime the library itself uses (torch bundles a second one, which finds no GPU after libbnhip's)
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipFree.argtypes = [C.c_void_p]
        blocks = []

        def dev(nbytes):
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), nbytes) == 0
            blocks.append(p)
            return p
        cap, ws = host.flac_max_bytes(B, n, 0), host.flac_workspace_size(B, n)
        d_in, d_out, d_off, d_ws = dev(gained.nbytes), dev(cap), dev(8 * (B + 1)), dev(ws)
        assert hip.hipMemcpy(d_in, gained.ctypes.data, gained.nbytes, 1) == 0

        def leg_d():
            host.flac_encode_device(d_in, B, n, rate, d_out, cap, d_off, d_ws, ws)
            assert hip.hipDeviceSynchronize() == 0
        legs["d"] = leg_d
        if "g" in a.legs:
            ws_lpc = host.flac_lpc_workspace_size(B, n, M)
            d_out_lpc, d_off_lpc, d_ws_lpc = dev(cap), dev(8 * (B + 1)), dev(ws_lpc)

            def leg_g():
                host.flac_encode_device(d_in, B, n, rate, d_out_lpc, cap, d_off_lpc, d_ws_lpc, ws_lpc, lpc_order=M)
                assert hip.hipDeviceSynchronize() == 0
            legs["g"] = leg_g
    run = [l for l in "abcdfg" if l in a.legs]
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
    names = {"a": "a_normalize_pcm_back", "b": "b_normalize_flac", "c": "c_normalize_flac_per_clip", "d": "d_flac_device_resident",
             "f": "f_normalize_flac_lpc", "g": "g_flac_lpc_device_resident"}
    for l in run:
        v = np.array(ts[l])
        res[names[l] + "_ms"] = round(float(np.median(v)), 3)
        res[names[l] + "_min_ms"] = round(float(v.min()), 3)
        res[names[l] + "_pass_medians_ms"] = [round(float(np.median(h)), 3) for h in np.split(v, 2)]
    ok = True
    rec = B * C.sizeof(host.Loudness)
    res["compressed_bytes"] = total
    res["compression_ratio"] = round(total / pcm.nbytes, 4)
    ratios = [len(s) / (2.0 * n) for s in want_streams]
    res["compression_ratio_per_clip_min_median_max"] = [round(float(f(ratios)), 4) for f in (np.min, np.median, np.max)]
    # (e): (a) returns the records and every PCM byte; (b) the records, the offsets and exactly offsets[n_clips] bytes
    res["e_d2h_bytes_a"] = rec + int(pcm.nbytes)
    res["e_d2h_bytes_b"] = rec + 8 * (B + 1) + total
    res["e_d2h_bytes_b_without_offsets"] = rec + total
    res["e_d2h_b_over_a"] = round(res["e_d2h_bytes_b"] / res["e_d2h_bytes_a"], 4)
    if "b" in run:
        r, streams = got["b"]
        res["b_equals_a_then_encode"] = bool(fields(r) == fields(want_res) and streams == want_streams)
        res["b_clips_gate_lifted"] = sum(1 for g in r if g.flags & host.LOUDNESS_GATE_LIFTED)
        import flacdec
        res["b_clip0_decodes_to_a"] = bool(np.array_equal(flacdec.decode(streams[0])[0], gained[0]))
        # (e) of (b) from (b)'s own answer: the entry copies offsets, then exactly offsets[n_clips] = the streams' bytes, and the records
        written = sum(len(s) for s in streams)
        res["b_offsets_last"] = written
        res["e_b_equals_offsets_last_plus_records"] = bool(res["e_d2h_bytes_b_without_offsets"] == written + rec)
        ok = ok and res["b_equals_a_then_encode"] and res["b_clip0_decodes_to_a"] and res["e_b_equals_offsets_last_plus_records"]
        if "a" in run:
            res["b_over_a"] = round(res["b_normalize_flac_ms"] / res["a_normalize_pcm_back_ms"], 3)
    if "c" in run:
        res["c_equals_b"] = bool([s[0] for _, s in got["c"]] == want_streams and fields([r[0] for r, _ in got["c"]]) == fields(want_res))
        ok = ok and res["c_equals_b"]
        if "b" in run:
            res["speedup_b_over_c"] = round(res["c_normalize_flac_per_clip_ms"] / res["b_normalize_flac_ms"], 2)
    if "d" in run:
        off = np.zeros(B + 1, np.uint64)
        assert hip.hipMemcpy(off.ctypes.data, d_off, off.nbytes, 2) == 0
        out = np.empty(int(off[B]), np.uint8)
        assert hip.hipMemcpy(out.ctypes.data, d_out, out.nbytes, 2) == 0
        res["d_equals_b"] = bool(out.tobytes() == b"".join(want_streams))
        ok = ok and res["d_equals_b"]
        res["d_GB_per_s_of_pcm"] = round(pcm.nbytes / (res["d_flac_device_resident_ms"] / 1e3) / 1e9, 1)
    if want_lpc is not None:
        total_lpc = sum(len(s) for s in want_lpc)
        res["lpc_compressed_bytes"] = total_lpc
        res["lpc_compression_ratio"] = round(total_lpc / pcm.nbytes, 4)
        ratios = [len(s) / (2.0 * n) for s in want_lpc]
        res["lpc_compression_ratio_per_clip_min_median_max"] = [round(float(f(ratios)), 4) for f in (np.min, np.median, np.max)]
        res["e_d2h_bytes_f"] = rec + 8 * (B + 1) + total_lpc
        res["e_d2h_f_over_a"] = round(res["e_d2h_bytes_f"] / res["e_d2h_bytes_a"], 4)
    if "f" in run:
        r, streams = got["f"]
        import flaclpcdec
        res["f_equals_a_then_encode"] = bool(fields(r) == fields(want_res) and streams == want_lpc)
        res["f_clip0_decodes_to_a"] = bool(np.array_equal(flaclpcdec.decode(streams[0])[0], gained[0]))
        ok = ok and res["f_equals_a_then_encode"] and res["f_clip0_decodes_to_a"]
        if "b" in run:
            res["f_over_b"] = round(res["f_normalize_flac_lpc_ms"] / res["b_normalize_flac_ms"], 3)
    if "g" in run:
        off = np.zeros(B + 1, np.uint64)
        assert hip.hipMemcpy(off.ctypes.data, d_off_lpc, off.nbytes, 2) == 0
        out = np.empty(int(off[B]), np.uint8)
        assert hip.hipMemcpy(out.ctypes.data, d_out_lpc, out.nbytes, 2) == 0
        res["g_equals_f"] = bool(out.tobytes() == b"".join(want_lpc))
        ok = ok and res["g_equals_f"]
        res["g_GB_per_s_of_pcm"] = round(pcm.nbytes / (res["g_flac_lpc_device_resident_ms"] / 1e3) / 1e9, 1)
        if "d" in run:
            res["g_over_d"] = round(res["g_flac_lpc_device_resident_ms"] / res["d_flac_device_resident_ms"], 3)
    if "d" in a.legs or "g" in a.legs:
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
