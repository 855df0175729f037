"""Cost of the loudness normalisation of a burst of detections: 64 clips of 15 s at 48 kHz, the export plan
(-23 LUFS, -1 dBTP, +-60 dB, gate fallback), output applied:
  (a) one bnhip_loudness_normalize_pcm16 call per clip (the shape of the reference's one measurement per saved clip);
  (b) one call for all clips;
  (c) tools/loudness_ref.c on ONE CPU thread over --cpu-clips clips, scaled to the 64: a float32 C RESTATEMENT of the reference's
      meter, plan and gain written for this project - NOT the reference's Go, whose SIMD library is not on this machine;
  (d) bnhip_loudness_normalize_device on clips, outputs and workspace already on the device, synchronised: (b) without its
      allocations and host copies.
Host clock around calls that end in a synchronise; --warmup warm-up and --reps timed repetitions per leg, the legs alternated
twice (half the repetitions per pass).  (a), (b) and (d) are compared field for field and byte for byte, (c) within the float32
distance the tests allow (1e-3 LU, 1e-3 dBTP).  Prints one JSON line and writes it to --out.

    python tools/loudness_rate.py [--clips 64] [--seconds 15] [--reps 20] [--warmup 3] [--legs abcd] [--out profiles/r13_loudness_rate.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import birdnet_go_amd  # noqa: E402,F401
from birdnet_go_amd import host  # noqa: E402

PLAN = dict(target_lufs=-23.0, true_peak_dbtp=-1.0, max_gain_db=60.0, gate_fallback=True)


def clips_48k(n_clips, seconds, rate=48000, seed=3):
    """Detection-like material: a few drifting tones over low noise per clip at levels 40 dB apart, int16; every eighth clip is a
    sub-gate noise floor (the gate fallback's case)."""
    rng = np.random.default_rng(seed)
    n = seconds * rate
    t = np.arange(n) / rate
    out = np.empty((n_clips, n), np.int16)
    for i in range(n_clips):
        if i % 8 == 7:
            out[i] = rng.integers(-3, 4, n)
            continue
        x = 0.003 * rng.standard_normal(n)
        for _ in range(4):
            f0, f1 = rng.uniform(1500.0, 9000.0, 2)
            x += rng.uniform(0.02, 0.3) * np.sin(2.0 * np.pi * (f0 * t + (f1 - f0) * t * t / (2.0 * seconds)))
        out[i] = np.round(np.clip(x * 10.0 ** (-rng.uniform(0.0, 40.0) / 20.0), -1.0, 1.0) * 32767.0).astype(np.int16)
    return out


def fields(res):
    return [tuple(getattr(g, f) for f, _ in host.Loudness._fields_) for g in res]


def c_restatement():
    """tools/loudness_ref.c built into a temporary directory -> the loaded library (kept alive with its directory)."""
    d = tempfile.mkdtemp(prefix="loudref_")
    so = os.path.join(d, "libloudref.so")
    subprocess.check_call(["gcc", "-O3", "-march=native", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tools", "loudness_ref.c"),
                           "-o", so, "-lm"])
    lib = C.CDLL(so)
    lib.loudref_normalize.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_double, C.c_double,
                                      C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-clips", type=int, default=4)
    ap.add_argument("--legs", default="abcd")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_loudness_rate.json"))
    a = ap.parse_args()
    host.init()                                                      # no device: a loud error, not a fallback
    rate = 48000
    pcm = clips_48k(a.clips, a.seconds, rate)
    B, n = pcm.shape
    res = {"tool": "loudness_rate", "clips": B, "seconds": a.seconds, "rate": rate, "plan": PLAN, "reps": a.reps, "warmup": a.warmup,
           "sub_blocks_per_clip": n // host.loudness_sub_block(rate), "bytes_in_per_clip": n * 2, "bytes_out_per_clip": n * 2}

    def call(x):
        return host.loudness_normalize(x, rate, PLAN["target_lufs"], PLAN["true_peak_dbtp"], PLAN["max_gain_db"], PLAN["gate_fallback"])

    def leg_a():
        r = [call(c) for c in pcm]
        return [g[0][0] for g in r], np.concatenate([g[1] for g in r])

    legs = {"a": leg_a, "b": lambda: call(pcm)}
    if "d" in a.legs:
        # device memory through the HIP runtime the library itself uses (torch bundles a second one, which finds no GPU after libbnhip's)
        hip = C.CDLL("libamdhip64.so")

        def dev(nbytes):
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
            return p
        ws = host.loudness_workspace_size(B, n, rate)
        d_in, d_out, d_res, d_ws = dev(pcm.nbytes), dev(pcm.nbytes), dev(B * C.sizeof(host.Loudness)), dev(ws)
        assert hip.hipMemcpy(d_in, C.c_void_p(pcm.ctypes.data), C.c_size_t(pcm.nbytes), 1) == 0

        def leg_d():
            host.loudness_normalize_device(d_in, B, n, rate, d_res, d_ws, ws, d_out, PLAN["target_lufs"], PLAN["true_peak_dbtp"],
                                           PLAN["max_gain_db"], PLAN["gate_fallback"])
            assert hip.hipDeviceSynchronize() == 0
        legs["d"] = leg_d
    run = [l for l in "abd" if l in a.legs]
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
    names = {"a": "a_one_call_per_clip", "b": "b_one_call", "d": "d_device_resident"}
    for l in run:
        v = np.array(ts[l])
        res[names[l] + "_ms"] = round(float(np.median(v)), 3)
        res[names[l] + "_min_ms"] = round(float(v.min()), 3)
        res[names[l] + "_pass_medians_ms"] = [round(float(np.median(h)), 3) for h in np.split(v, 2)]
        res[names[l] + "_clips_per_s"] = round(B / (float(np.median(v)) / 1e3))
    ok = True
    if "a" in run and "b" in run:
        res["speedup_b_over_a"] = round(res["a_one_call_per_clip_ms"] / res["b_one_call_ms"], 2)
        res["a_equals_b"] = bool(fields(got["a"][0]) == fields(got["b"][0]) and np.array_equal(got["a"][1], got["b"][1]))
        ok = ok and res["a_equals_b"]
    if "b" in run:
        r = got["b"][0]
        res["b_clips_gate_lifted"] = sum(1 for g in r if g.flags & host.LOUDNESS_GATE_LIFTED)
        res["b_host_copy_MB"] = round(B * n * 4 / 1e6, 1)
    if "b" in run and "d" in run:
        dres, dout = (host.Loudness * B)(), np.empty_like(pcm)
        assert hip.hipMemcpy(C.c_void_p(C.addressof(dres)), d_res, C.c_size_t(C.sizeof(dres)), 2) == 0
        assert hip.hipMemcpy(C.c_void_p(dout.ctypes.data), d_out, C.c_size_t(dout.nbytes), 2) == 0
        res["d_equals_b"] = bool(fields(dres) == fields(got["b"][0]) and np.array_equal(dout, got["b"][1]))
        ok = ok and res["d_equals_b"]
        res["b_share_outside_kernels"] = round(1.0 - res["d_device_resident_ms"] / res["b_one_call_ms"], 3)
    if "c" in a.legs:
        import loudref as R
        lib = c_restatement()
        kw = np.array(R.kweight64(rate), np.float32)
        tp = np.ascontiguousarray(R.tp_coef64().astype(np.float32))
        k = min(a.cpu_clips, B)
        idx = [7 % B] + [i for i in range(B) if i % 8 != 7][:max(0, k - 1)]           # one lifted clip among them, as in the burst
        share = res.get("b_clips_gate_lifted", B // 8) / B                            # of lifted clips: they are measured twice
        out, r3 = np.empty(n, np.int16), np.zeros(3)
        ms, cres = {}, {}
        for i in idx:
            t0 = time.perf_counter()
            rc = lib.loudref_normalize(pcm[i].ctypes.data, n, rate, kw.ctypes.data, tp.ctypes.data, np.float32(R.GATE_ABS), np.float32(R.GATE_REL),
                                       PLAN["target_lufs"], PLAN["true_peak_dbtp"], PLAN["max_gain_db"], 1, out.ctypes.data, r3.ctypes.data)
            ms[i] = (time.perf_counter() - t0) * 1e3
            assert rc == 0
            cres[i] = r3.copy()
        lifted = [ms[i] for i in idx if i % 8 == 7]
        plain = [ms[i] for i in idx if i % 8 != 7] or lifted
        per_clip = share * float(np.mean(lifted)) + (1.0 - share) * float(np.mean(plain))
        res["c_clips_timed"] = len(idx)
        res["c_ms_per_plain_clip"] = round(float(np.mean(plain)), 2)
        res["c_ms_per_lifted_clip"] = round(float(np.mean(lifted)), 2)
        res["c_restatement_one_thread_ms_scaled"] = round(per_clip * B, 1)
        res["c_is"] = "float32 C restatement of the reference's meter, plan and gain (tools/loudness_ref.c), one CPU thread; not the reference's Go"
        if "b" in run:
            res["speedup_b_over_c"] = round(res["c_restatement_one_thread_ms_scaled"] / res["b_one_call_ms"], 1)
            dl = dp = dg = 0.0
            for i in idx:
                g = got["b"][0][i]
                if np.isfinite(g.integrated_lufs) or np.isfinite(cres[i][0]):
                    dl = max(dl, abs(g.integrated_lufs - cres[i][0]))
                dp = max(dp, abs(g.true_peak_dbtp - cres[i][1]))
                dg = max(dg, abs(g.gain_db - cres[i][2]))
            res["b_vs_c_max_abs"] = {"lufs": float(f"{dl:.3g}"), "dbtp": float(f"{dp:.3g}"), "gain_db": float(f"{dg:.3g}")}
            res["b_within_1e-3_of_c"] = bool(dl <= 1e-3 and dp <= 1e-3 and dg <= 2e-3)
            ok = ok and res["b_within_1e-3_of_c"]
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
