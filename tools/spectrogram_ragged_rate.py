"""Cost of the spectrogram PNG files of a burst of detections of unequal lengths ("ragged spectrograms"): 64 clips at
48 kHz with 64 distinct lengths between 9 s and 45 s (tools/ragged_rate.py's burst, seed 16), material from
tools/spectrogram_rate.py's generator, bird profile (resampled to 24 kHz on the device), "lg" (1026 x 513, N = 1024), default style:
  (r) bnhip_spectrogram_png_ragged_pcm16, the whole burst in one call;
  (g) the grouped path, one bnhip_spectrogram_png_pcm16 call per distinct length - here one per clip;
  (i) bnhip_spectrogram_ragged_pcm16, the render without the encoder, and (s) its render kernel alone on the device-resident packed
      float32 through bnhip_spectrogram_ragged_device, by HIP events: where the call's time goes;
  (u) bnhip_spectrogram_pcm16 on tools/spectrogram_rate.py's uniform burst (64 clips of 15 s) and (k) its render kernel alone through
      bnhip_spectrogram_device, by HIP events - the guards that show what the uniform path pays for the per-clip geometry.
The library is the one host.py loads: BNHIP_LIB names another build, so the same tool run against the parent commit's library
(--legs guk: it has no ragged entry) gives the baseline and the guards' other side.  Host clock around calls that end in a
synchronise; --warmup warm-up and --reps timed repetitions per leg, the legs alternated twice (half the repetitions per pass).
(r) is checked against (g) in every byte.  Prints one JSON line and writes it to --out.

    python tools/spectrogram_ragged_rate.py [--legs rgisuk] [--reps 20] [--warmup 3] [--seed 16] [--out profiles/r18_spec_ragged_rate.json]
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
from birdnet_go_amd import host, spectrogram as sg  # noqa: E402
from ragged_rate import burst_lengths  # noqa: E402
from spectrogram_rate import clips_48k  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--size", default="lg")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="rgisuk")
    ap.add_argument("--seed", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_spec_ragged_rate.json"))
    a = ap.parse_args()
    host.init()                                                      # no device: a loud error, not a fallback
    rate, rate_out = 48000, sg.bird_profile().resample_rate
    width = sg.size_to_pixels(a.size)
    height, fft = host.spectrogram_size(width)
    pal = sg.palette("default")
    lens = burst_lengths(a.clips, rate, a.seed)
    long_clips = clips_48k(a.clips, 45, rate)
    burst = [np.ascontiguousarray(long_clips[i, :n]) for i, n in enumerate(lens)]
    uniform = np.ascontiguousarray(long_clips[:, :15 * rate])
    del long_clips
    with open(host.LIB_PATH, "rb") as fh:
        digest = hashlib.sha256(fh.read()).hexdigest()[:16]
    res = {"tool": "spectrogram_ragged_rate", "library": os.path.relpath(host.LIB_PATH, ROOT), "library_sha256_16": digest, "clips": a.clips,
           "rate_in": rate, "rate_out": rate_out, "seed": a.seed, "lengths": lens, "distinct_lengths": len(set(lens)),
           "pcm_bytes": int(2 * sum(lens)), "width": width, "height": height, "fft_size": fft, "image_bytes": a.clips * width * height,
           "reps": a.reps, "warmup": a.warmup, "uniform_clips_seconds": [a.clips, 15]}
    legs = {"g": lambda: [host.spectrogram_png(c, rate, width, pal, rate_out=rate_out)[0] for c in burst],
            "u": lambda: host.spectrogram(uniform, rate, width, rate_out=rate_out)}
    if "r" in a.legs:
        legs["r"] = lambda: host.spectrogram_png_ragged(burst, rate, width, pal, rate_out=rate_out)
    if "i" in a.legs:
        legs["i"] = lambda: host.spectrogram_ragged(burst, rate, width, rate_out=rate_out)
    blocks, events = [], {}
    if "k" in a.legs or "s" in a.legs:
        # device memory and events through the HIP runtime the library itself uses
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipFree.argtypes = [C.c_void_p]
        hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        hip.hipEventSynchronize.argtypes = [C.c_void_p]
        hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        hip.hipEventDestroy.argtypes = [C.c_void_p]
        e0, e1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0

        def dev(nbytes, src=None):
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), nbytes) == 0
            blocks.append(p)
            if src is not None:
                assert hip.hipMemcpy(p, src.ctypes.data, src.nbytes, 1) == 0
            return p

        def timed(enqueue):
            """-> milliseconds between two events around what `enqueue` puts on the default stream"""
            def leg():
                assert hip.hipEventRecord(e0, None) == 0
                enqueue()
                assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
                ms = C.c_float(0.0)
                assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
                return ms.value
            return leg
        rs = host.Resampler(rate, rate_out)
        to_f32 = lambda x: rs.resample_f32(x.astype(np.float32) / np.float32(32768.0))
    if "k" in a.legs:
        f32 = np.ascontiguousarray(to_f32(uniform))
        B, n = f32.shape
        d_in, d_img = dev(f32.nbytes, f32), dev(B * height * width)
        events["k"] = timed(lambda: host.spectrogram_device(d_in, True, B, n, width, height, d_img))
        del f32
    if "s" in a.legs:
        parts = [to_f32(c[None, :])[0] for c in burst]
        packed, rl = np.ascontiguousarray(np.concatenate(parts)), [p.size for p in parts]
        ws = host.spectrogram_ragged_workspace_size(rl, width)
        d_rin, d_rimg, d_ws = dev(packed.nbytes, packed), dev(a.clips * height * width), dev(ws)
        events["s"] = timed(lambda: host.spectrogram_ragged_device(d_rin, True, rl, width, height, d_rimg, d_ws, ws))
        res["rendered_samples"] = int(sum(rl))
        del packed, parts
    run = [l for l in "rgisuk" if l in a.legs and (l in legs or l in events)]
    ts, got = {l: [] for l in run}, {}
    for l in run:
        for _ in range(a.warmup):
            (legs.get(l) or events[l])()
    for p in range(2):                                               # the legs alternated twice
        for l in run:
            for _ in range(a.reps // 2):
                if l in events:
                    ts[l].append(events[l]())
                    continue
                t0 = time.perf_counter()
                got[l] = legs[l]()
                ts[l].append((time.perf_counter() - t0) * 1e3)
    names = {"r": "r_ragged_png_one_call", "g": "g_grouped_png_per_length", "i": "i_ragged_render_one_call", "s": "s_ragged_render_kernel_events",
             "u": "u_uniform_render", "k": "k_uniform_render_kernel_events"}
    for l in run:
        v = np.array(ts[l])
        res[names[l] + "_ms"] = round(float(np.median(v)), 3)
        res[names[l] + "_min_ms"] = round(float(v.min()), 3)
        res[names[l] + "_pass_medians_ms"] = [round(float(np.median(h)), 3) for h in np.split(v, 2)]
    ok = True
    if "r" in run:
        res["png_bytes"] = sum(len(s) for s in got["r"])
    if "r" in run and "g" in run:
        res["r_equals_g"] = bool(got["r"] == got["g"])
        res["speedup_r_over_g"] = round(res["g_grouped_png_per_length_ms"] / res["r_ragged_png_one_call_ms"], 2)
        ok = ok and res["r_equals_g"]
    if "i" in run and "s" in run:
        res["s_kernel_share_of_i"] = round(res["s_ragged_render_kernel_events_ms"] / res["i_ragged_render_one_call_ms"], 3)
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
