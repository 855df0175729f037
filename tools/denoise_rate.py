"""Cost of the processed-audio entries ("Denoise"): a burst of 64 clips of 15 s at 48 kHz (material from
tools/spectrogram_rate.py's generator), medium preset, N = 2048:
  (d) bnhip_denoise_pcm16, the burst in one call: PCM up, PCM back;
  (k) k_denoise alone on device-resident clips through bnhip_denoise_device, by HIP events;
  (c) bnhip_process_pcm16 with all three stages (denoise, normalise to -23 LUFS / -2 dBTP, +3 dB);
  (l) bnhip_loudness_normalize_pcm16 of the same burst (no clamp, no fallback): what the chain adds to normalisation alone;
  (r) the float64 restatement tests/dnref.py, clip after clip on one host thread: the CPU baseline (--ref-clips of the burst,
      scaled to the whole burst).
The entries are called through ctypes on buffers prepared once, so a leg times the C call and not the Python wrapper.  Host clock
around calls that end in a synchronise; --warmup warm-up and --reps timed repetitions per leg, the legs alternated twice.  (d) and
(k) are compared with each other in every byte and with the restatement on the --ref-clips clips under its acceptance rule; (c) is
compared with the stages called one after another.  Prints one JSON line and writes it to --out.

    python tools/denoise_rate.py [--legs dkclr] [--reps 20] [--warmup 3] [--out profiles/r20_denoise_rate.json]
"""
import argparse
import ctypes as C
import hashlib
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import birdnet_go_amd  # noqa: E402,F401
import dnref  # noqa: E402
from birdnet_go_amd import host, loudness, process  # noqa: E402
from spectrogram_rate import clips_48k  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=int, default=15)
    ap.add_argument("--preset", default="medium")
    ap.add_argument("--gain-db", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-clips", type=int, default=4)
    ap.add_argument("--legs", default="dkclr")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_denoise_rate.json"))
    a = ap.parse_args()
    host.init()                                                      # no device: a loud error, not a fallback
    lib = host.load_library()
    lib.bnhip_last_error.restype = C.c_char_p
    rate = 48000
    frame = process.frame_for_rate(rate)
    nr, nf = (float(v) for v in process.DENOISE_PRESETS[a.preset])
    x = clips_48k(a.clips, a.seconds, rate)
    B, n = x.shape
    with open(host.LIB_PATH, "rb") as fh:
        digest = hashlib.sha256(fh.read()).hexdigest()[:16]
    res = {"tool": "denoise_rate", "library": os.path.relpath(host.LIB_PATH, ROOT), "library_sha256_16": digest, "clips": B, "rate": rate,
           "seconds": a.seconds, "samples_per_clip": n, "pcm_bytes": int(x.nbytes), "preset": a.preset, "nr_db": nr, "nf_db": nf, "frame": frame,
           "frames_per_clip": dnref.frame_count(n, frame), "gain_db": a.gain_db, "reps": a.reps, "warmup": a.warmup}
    vp, ci, sz, cd = C.c_void_p, C.c_int, C.c_size_t, C.c_double
    out_d, out_c, out_l = np.empty_like(x), np.empty_like(x), np.empty_like(x)
    rec_c, rec_l = (host.Loudness * B)(), (host.Loudness * B)()
    lib.bnhip_denoise_pcm16.argtypes = [ci, vp, ci, ci, ci, cd, cd, vp]
    lib.bnhip_process_pcm16.argtypes = [ci, vp, ci, ci, ci, ci, cd, cd, ci, cd, cd, cd, vp, vp]
    lib.bnhip_loudness_normalize_pcm16.argtypes = [ci, vp, ci, ci, ci, cd, cd, cd, ci, vp, vp]

    def check(rc):
        if rc != host.BNHIP_OK:
            raise SystemExit(f"entry failed: {rc} {lib.bnhip_last_error()}")

    legs = {
        "d": lambda: check(lib.bnhip_denoise_pcm16(0, x.ctypes.data, B, n, frame, nr, nf, out_d.ctypes.data)),
        "c": lambda: check(lib.bnhip_process_pcm16(0, x.ctypes.data, B, n, rate, frame, nr, nf, 1, -23.0, -2.0, a.gain_db, out_c.ctypes.data,
                                                   C.addressof(rec_c))),
        "l": lambda: check(lib.bnhip_loudness_normalize_pcm16(0, x.ctypes.data, B, n, rate, -23.0, -2.0, math.inf, 0, out_l.ctypes.data,
                                                              C.addressof(rec_l))),
    }
    blocks, events = [], {}
    if "k" in a.legs:
        # device memory and events through the HIP runtime the library itself uses
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(vp), sz]
        hip.hipMemcpy.argtypes = [vp, vp, sz, ci]
        hip.hipFree.argtypes = [vp]
        hip.hipEventCreate.argtypes = [C.POINTER(vp)]
        hip.hipEventRecord.argtypes = [vp, vp]
        hip.hipEventSynchronize.argtypes = [vp]
        hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
        hip.hipEventDestroy.argtypes = [vp]
        e0, e1 = vp(), vp()
        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0

        def dev(nbytes, src=None):
            p = vp()
            assert hip.hipMalloc(C.byref(p), nbytes) == 0
            blocks.append(p)
            if src is not None:
                assert hip.hipMemcpy(p, src.ctypes.data, src.nbytes, 1) == 0
            return p

        ws = host.denoise_workspace_size(B, n, frame)
        d_in, d_out, d_ws = dev(x.nbytes, x), dev(x.nbytes), dev(ws)

        def kernel():
            assert hip.hipEventRecord(e0, None) == 0
            host.denoise_device(d_in, B, n, frame, nr, nf, d_out, d_ws, ws)
            assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
            ms = C.c_float(0.0)
            assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
            return ms.value
        events["k"] = kernel
    run = [l for l in "dkcl" if l in a.legs]
    ts = {l: [] for l in run}
    for l in run:
        for _ in range(a.warmup):
            (legs.get(l) or events[l])()
    for _ in range(2):                                               # the legs alternated twice
        for l in run:
            for _ in range(a.reps // 2):
                if l in events:
                    ts[l].append(events[l]())
                    continue
                t0 = time.perf_counter()
                legs[l]()
                ts[l].append((time.perf_counter() - t0) * 1e3)
    names = {"d": "d_denoise_pcm16_one_call", "k": "k_denoise_kernel_events", "c": "c_process_three_stages_one_call",
             "l": "l_loudness_normalize_one_call"}
    for l in run:
        v = np.array(ts[l])
        res[names[l] + "_ms"] = round(float(np.median(v)), 3)
        res[names[l] + "_min_ms"] = round(float(v.min()), 3)
        res[names[l] + "_pass_medians_ms"] = [round(float(np.median(h)), 3) for h in np.split(v, 2)]
    ok = True
    audio_s = B * a.seconds
    if "d" in run:
        res["d_audio_seconds_per_second"] = round(audio_s / res[names["d"] + "_ms"] * 1e3, 1)
    if "k" in run:
        got = np.empty_like(x)
        assert hip.hipMemcpy(got.ctypes.data, d_out, got.nbytes, 2) == 0
        res["k_audio_seconds_per_second"] = round(audio_s / res[names["k"] + "_ms"] * 1e3, 1)
        res["k_frames_per_second"] = round(B * res["frames_per_clip"] / res[names["k"] + "_ms"] * 1e3, 1)
        if "d" in run:
            res["k_equals_d"] = bool(np.array_equal(got, out_d))
            res["d_host_copy_and_call_share"] = round(1.0 - res[names["k"] + "_ms"] / res[names["d"] + "_ms"], 3)
            ok = ok and res["k_equals_d"]
    if "c" in run:
        # the stages one after another, through the Python bindings (not timed)
        want = host.denoise(x, frame, nr, nf)
        want_rec, want = host.loudness_normalize(want, rate, -23.0, -2.0, math.inf, False)
        want = dnref.quant(want.astype(np.float64) * loudness.factor_from_db(a.gain_db))
        res["c_equals_stages"] = bool(np.array_equal(out_c, want) and all(p.factor == q.factor for p, q in zip(rec_c, want_rec)))
        ok = ok and res["c_equals_stages"]
        if "l" in run:
            res["c_over_l"] = round(res[names["c"] + "_ms"] / res[names["l"] + "_ms"], 3)
    if "r" in a.legs:
        m = max(1, min(a.ref_clips, B))
        t0 = time.perf_counter()
        ref = [dnref.denoise(x[i], frame, nr, nf) for i in range(m)]
        dt = (time.perf_counter() - t0) * 1e3
        res["r_restatement_clips_timed"] = m
        res["r_restatement_one_thread_ms_per_clip"] = round(dt / m, 3)
        res["r_restatement_one_thread_burst_ms"] = round(dt / m * B, 1)
        if "d" in run:
            v = np.stack(ref)
            dnref.compare(out_d[:m], x[:m], frame, nr, nf, restated=(dnref.quant(v), v))
            res["d_matches_restatement_on_timed_clips"] = True
            res["r_over_d"] = round(res["r_restatement_one_thread_burst_ms"] / res[names["d"] + "_ms"], 1)
    if events:
        for p in blocks:
            hip.hipFree(p)
        hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
