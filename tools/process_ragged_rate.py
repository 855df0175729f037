"""Cost of the processed spectrograms of a burst of detections of unequal lengths ("Denoise": ragged bursts and the
fused render): 64 clips at 48 kHz with 64 distinct lengths between 9 s and 45 s (tools/spectrogram_ragged_rate.py's burst, seed 16),
medium preset (N = 2048), normalised to -23 LUFS / -2 dBTP, +3 dB, then the bird profile's render (resampled to 24 kHz on the
device) at "lg" (1026 x 513), default style, PNG-encoded on the device:
  (f) bnhip_process_spectrogram_png_ragged_pcm16, the whole burst in one call: PCM up, PNG files back;
  (t) bnhip_process_ragged_pcm16, then bnhip_spectrogram_png_ragged_pcm16: two calls, the processed PCM through the host;
  (g) what a caller has without the ragged chain: per distinct length (here per clip) one bnhip_process_pcm16 and one
      bnhip_spectrogram_png_pcm16.  It uses only entries the previous release has, so BNHIP_LIB=<that build> --legs g gives the baseline;
  (k) ragged k_denoise alone on the device-resident packed clips through bnhip_denoise_ragged_device, by HIP events.
The entries are called through ctypes on buffers prepared once, so a leg times the C calls and not the Python wrappers.  Host clock
around calls that end in a synchronise; --warmup warm-up and --reps timed repetitions per leg, the legs alternated twice.  (f)'s PNG
bytes are compared with (t)'s and (g)'s clip by clip, where those legs run; a difference is exit status 1.  Prints one JSON line and
writes it to --out.

    python tools/process_ragged_rate.py [--legs ftgk] [--reps 10] [--warmup 2] [--seed 16] [--out profiles/r21_process_ragged_rate.json]
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
from birdnet_go_amd import host, process, spectrogram as sg  # noqa: E402
from ragged_rate import burst_lengths  # noqa: E402
from spectrogram_rate import clips_48k  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--size", default="lg")
    ap.add_argument("--preset", default="medium")
    ap.add_argument("--gain-db", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="ftgk")
    ap.add_argument("--seed", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_process_ragged_rate.json"))
    a = ap.parse_args()
    host.init()                                                      # no device: a loud error, not a fallback
    lib = host.load_library()
    rate, rate_out = 48000, sg.bird_profile().resample_rate
    frame = process.frame_for_rate(rate)
    nr, nf = (float(v) for v in process.DENOISE_PRESETS[a.preset])
    tl, tp = process.LOUDNORM_TARGET_I, process.LOUDNORM_TARGET_TP
    width = sg.size_to_pixels(a.size)
    height, fft = host.spectrogram_size(width)
    kw = sg._render_args(rate, width, None, "default", "100")
    keep, wp = host._spectrogram_window(kw["window"], fft)
    top_db, range_db = float(kw["top_db"]), float(kw["range_db"])
    pal = host._png_palette(sg.palette("default"))
    lens = burst_lengths(a.clips, rate, a.seed)
    long_clips = clips_48k(a.clips, 45, rate)
    burst = [np.ascontiguousarray(long_clips[i, :n]) for i, n in enumerate(lens)]
    del long_clips
    x, lens32 = host.ragged_pack(burst)
    B = int(lens32.size)
    with open(host.LIB_PATH, "rb") as fh:
        digest = hashlib.sha256(fh.read()).hexdigest()[:16]
    res = {"tool": "process_ragged_rate", "library": os.path.relpath(host.LIB_PATH, ROOT), "library_sha256_16": digest, "clips": B,
           "rate_in": rate, "rate_out": rate_out, "seed": a.seed, "lengths": lens, "distinct_lengths": len(set(lens)),
           "pcm_bytes": int(x.nbytes), "audio_seconds": round(x.size / rate, 1), "preset": a.preset, "nr_db": nr, "nf_db": nf, "frame": frame,
           "target_lufs": tl, "true_peak_dbtp": tp, "gain_db": a.gain_db, "width": width, "height": height, "fft_size": fft, "reps": a.reps,
           "warmup": a.warmup}
    vp, ci, sz, cd = C.c_void_p, C.c_int, C.c_size_t, C.c_double
    cap, cap1 = host.png_max_bytes(B, width, height), host.png_max_bytes(1, width, height)
    rec = (host.Loudness * B)()
    lib.bnhip_process_pcm16.argtypes = [ci, vp, ci, ci, ci, ci, cd, cd, ci, cd, cd, cd, vp, vp]
    lib.bnhip_spectrogram_png_pcm16.argtypes = [ci, vp, ci, ci, ci, ci, ci, ci, vp, cd, cd, vp, vp, sz, vp]
    if set("ftk") & set(a.legs):
        lib.bnhip_process_ragged_pcm16.argtypes = [ci, vp, ci, vp, ci, ci, cd, cd, ci, cd, cd, cd, vp, vp]
        lib.bnhip_spectrogram_png_ragged_pcm16.argtypes = [ci, vp, ci, vp, ci, ci, ci, ci, vp, cd, cd, vp, vp, sz, vp]
        lib.bnhip_process_spectrogram_png_ragged_pcm16.argtypes = [ci, vp, ci, vp, ci, ci, cd, cd, ci, cd, cd, cd, ci, ci, ci, vp, cd, cd, vp, vp,
                                                                   sz, vp, vp, vp]

    def check(rc):
        if rc != host.BNHIP_OK:
            raise SystemExit(f"entry failed: {rc} {lib.bnhip_last_error()}")

    out_f, off_f = np.empty(cap, np.uint8), np.zeros(B + 1, np.uint64)
    out_t, off_t, pcm_t = np.empty(cap, np.uint8), np.zeros(B + 1, np.uint64), np.empty_like(x)
    out_g, off_g, pcm_g = np.empty((B, cap1), np.uint8), np.zeros((B, 2), np.uint64), np.empty(max(lens), np.int16)
    starts = np.concatenate([[0], np.cumsum(lens32.astype(np.int64))])

    def leg_f():
        check(lib.bnhip_process_spectrogram_png_ragged_pcm16(0, x.ctypes.data, B, lens32.ctypes.data, rate, frame, nr, nf, 1, tl, tp, a.gain_db,
                                                             rate_out, width, height, wp, top_db, range_db, pal.ctypes.data, out_f.ctypes.data,
                                                             cap, off_f.ctypes.data, C.addressof(rec), None))

    def leg_t():
        check(lib.bnhip_process_ragged_pcm16(0, x.ctypes.data, B, lens32.ctypes.data, rate, frame, nr, nf, 1, tl, tp, a.gain_db, pcm_t.ctypes.data,
                                             C.addressof(rec)))
        check(lib.bnhip_spectrogram_png_ragged_pcm16(0, pcm_t.ctypes.data, B, lens32.ctypes.data, rate, rate_out, width, height, wp, top_db,
                                                     range_db, pal.ctypes.data, out_t.ctypes.data, cap, off_t.ctypes.data))

    def leg_g():
        for i in range(B):                                           # (64 distinct lengths: a group is one clip)
            n = int(lens32[i])
            check(lib.bnhip_process_pcm16(0, x.ctypes.data + 2 * int(starts[i]), 1, n, rate, frame, nr, nf, 1, tl, tp, a.gain_db,
                                          pcm_g.ctypes.data, C.addressof(rec) + i * C.sizeof(host.Loudness)))
            check(lib.bnhip_spectrogram_png_pcm16(0, pcm_g.ctypes.data, 1, n, rate, rate_out, width, height, wp, top_db, range_db,
                                                  pal.ctypes.data, out_g[i].ctypes.data, cap1, off_g[i].ctypes.data))

    legs = {"f": leg_f, "t": leg_t, "g": leg_g}
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

        ws = host.denoise_ragged_workspace_size(lens32, frame)
        d_in, d_out, d_ws = dev(x.nbytes, x), dev(x.nbytes), dev(ws)

        def kernel():
            assert hip.hipEventRecord(e0, None) == 0
            host.denoise_ragged_device(d_in, lens32, frame, nr, nf, d_out, d_ws, ws)
            assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
            ms = C.c_float(0.0)
            assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
            return ms.value
        events["k"] = kernel
    run = [l for l in "ftgk" if l in a.legs]
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
    names = {"f": "f_fused_one_call", "t": "t_two_ragged_calls", "g": "g_two_calls_per_length", "k": "k_denoise_ragged_kernel_events"}
    for l in run:
        v = np.array(ts[l])
        res[names[l] + "_ms"] = round(float(np.median(v)), 3)
        res[names[l] + "_min_ms"] = round(float(v.min()), 3)
        res[names[l] + "_pass_medians_ms"] = [round(float(np.median(h)), 3) for h in np.split(v, 2)]
    png = {}
    if "f" in run:
        png["f"] = [out_f[int(off_f[i]):int(off_f[i + 1])].tobytes() for i in range(B)]
    if "t" in run:
        png["t"] = [out_t[int(off_t[i]):int(off_t[i + 1])].tobytes() for i in range(B)]
    if "g" in run:
        png["g"] = [out_g[i, :int(off_g[i, 1])].tobytes() for i in range(B)]
    for l, streams in png.items():
        res[l + "_png_bytes"] = sum(len(s) for s in streams)
        res[l + "_png_sha256_16"] = hashlib.sha256(b"".join(streams)).hexdigest()[:16]
    ok = True
    for l in ("t", "g"):
        if "f" in png and l in png:
            res[f"f_equals_{l}"] = bool(all(p == q for p, q in zip(png["f"], png[l])) and len(png["f"]) == len(png[l]))
            res[f"speedup_f_over_{l}"] = round(res[names[l] + "_ms"] / res[names["f"] + "_ms"], 2)
            ok = ok and res[f"f_equals_{l}"]
    if "k" in run:
        res["k_audio_seconds_per_second"] = round(res["audio_seconds"] / res[names["k"] + "_ms"] * 1e3, 1)
    if events:
        for p in blocks:
            hip.hipFree(p)
        hip.hipEventDestroy(e0); hip.hipEventDestroy(e1)
    del keep
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
