"""Cost of the spectrogram images of a burst of detections, three ways: 64 clips of 15 s at 48 kHz, bird profile
(resampled to 24 kHz on the device), "lg" (1026 x 513, N = 1024):
  (a) one bnhip_spectrogram_pcm16 call per clip (the shape of the reference's one `sox` child per image, generator.go:425);
  (b) one call for all clips;
  (c) the float64 numpy restatement of the rendering spec (tests/specref.py) on ONE CPU thread over --cpu-clips clips of the
      device-resampled samples, scaled to the 64 - a RESTATEMENT of this project's spec, NOT sox (sox is not on this machine).
Host clock around calls that end in a synchronise; --warmup warm-up and --reps timed repetitions per leg, the legs alternated
twice (half the repetitions per pass).  The images of (a) and (b) are compared byte for byte, (c) under the tests' acceptance rule.
Prints one JSON line and writes it to --out.

    python tools/spectrogram_rate.py [--clips 64] [--seconds 15] [--reps 30] [--warmup 5] [--legs abc] [--out profiles/r10_spectrogram_rate.json]
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
from birdnet_go_amd import host, spectrogram as sg  # noqa: E402


def clips_48k(n_clips, seconds, rate=48000, seed=3):
    """Bird-band material: a few drifting tones over low noise per clip, int16."""
    rng = np.random.default_rng(seed)
    n = seconds * rate
    t = np.arange(n) / rate
    out = np.empty((n_clips, n), np.int16)
    for i in range(n_clips):
        x = 0.003 * rng.standard_normal(n)
        for _ in range(4):
            f0, f1 = rng.uniform(1500.0, 9000.0, 2)
            x += rng.uniform(0.02, 0.3) * np.sin(2.0 * np.pi * (f0 * t + (f1 - f0) * t * t / (2.0 * seconds)))
        out[i] = np.round(np.clip(x, -1.0, 1.0) * 32767.0).astype(np.int16)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=int, default=15)
    ap.add_argument("--size", default="lg")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-clips", type=int, default=4)
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_spectrogram_rate.json"))
    a = ap.parse_args()
    host.init()                                                      # no device: a loud error, not a fallback
    rate, prof = 48000, sg.bird_profile()
    width = sg.size_to_pixels(a.size)
    height, fft = host.spectrogram_size(width)
    pcm = clips_48k(a.clips, a.seconds, rate)
    n_render = host.Resampler(rate, prof.resample_rate).estimate_output(pcm.shape[1])
    res = {"tool": "spectrogram_rate", "clips": a.clips, "seconds": a.seconds, "rate_in": rate, "rate_out": prof.resample_rate,
           "width": width, "height": height, "fft_size": fft, "samples_rendered_per_clip": n_render,
           "hop": round(n_render / width, 1), "reps": a.reps, "warmup": a.warmup,
           "bytes_in_per_clip": int(pcm.shape[1] * 2), "bytes_out_per_clip": int(width * height)}

    legs = {"a": lambda: np.concatenate([host.spectrogram(c, rate, width, rate_out=prof.resample_rate) for c in pcm]),
            "b": lambda: host.spectrogram(pcm, rate, width, rate_out=prof.resample_rate)}
    run = [l for l in "ab" if l in a.legs]
    ts, img = {l: [] for l in run}, {}
    for l in run:
        for _ in range(a.warmup):
            legs[l]()
    for p in range(2):                                               # the legs alternated twice
        for l in run:
            for _ in range(a.reps // 2):
                t0 = time.perf_counter()
                img[l] = legs[l]()
                ts[l].append((time.perf_counter() - t0) * 1e3)
    names = {"a": "a_one_call_per_clip", "b": "b_one_call"}
    for l in run:
        v = np.array(ts[l])
        res[names[l] + "_ms"] = round(float(np.median(v)), 3)
        res[names[l] + "_min_ms"] = round(float(v.min()), 3)
        res[names[l] + "_pass_medians_ms"] = [round(float(np.median(h)), 3) for h in np.split(v, 2)]
        res[names[l] + "_clips_per_s"] = round(a.clips / (float(np.median(v)) / 1e3))
    ok = True
    if "a" in run and "b" in run:
        res["speedup_b_over_a"] = round(res["a_one_call_per_clip_ms"] / res["b_one_call_ms"], 2)
        res["a_equals_b"] = bool(np.array_equal(img["a"], img["b"]))
        ok = ok and res["a_equals_b"]
    if "b" in run:
        mb = a.clips * (res["bytes_in_per_clip"] + res["bytes_out_per_clip"]) / 1e6
        res["b_host_copy_MB"] = round(mb, 1)
        res["b_host_copy_GBps_if_copies_alone"] = round(mb / res["b_one_call_ms"], 2)
    if "c" in a.legs:
        import specref                                               # (numpy's FFT runs on the calling thread)
        k = min(a.cpu_clips, a.clips)
        f32 = host.Resampler(rate, prof.resample_rate).resample_f32(pcm[:k].astype(np.float32) / np.float32(32768.0))
        t0 = time.perf_counter()
        ref = [specref.render(f32[i].astype(np.float64), width, height) for i in range(k)]
        ms = (time.perf_counter() - t0) * 1e3
        res["c_numpy_restatement_clips_timed"] = k
        res["c_numpy_restatement_one_thread_ms_scaled"] = round(ms * a.clips / k, 1)
        res["c_is"] = "float64 numpy restatement of this project's rendering spec, one CPU thread; not sox"
        if "b" in run:
            res["speedup_b_over_c"] = round(res["c_numpy_restatement_one_thread_ms_scaled"] / res["b_one_call_ms"], 1)
            for i in range(k):
                specref.compare(img["b"][i], f32[i].astype(np.float64), width, height)
            res["b_meets_acceptance_rule_vs_c"] = True
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
