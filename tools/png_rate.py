"""Cost of the spectrogram PNG files of a burst of detections ("PNG"): tools/spectrogram_rate.py's burst - 64 clips
of 15 s at 48 kHz, bird profile (resampled to 24 kHz on the device), "lg" (1026 x 513) - all legs in one process:
  (a) what existed before: bnhip_spectrogram_pcm16, then zlib level 6 per image on ONE host thread, in memory (the chunks of
      spectrogram.write_png without the file); the render and the compression are also timed apart;
  (b) bnhip_spectrogram_png_pcm16: render and encode in one device call, the streams returned;
  (c) the encoder's kernels alone on device-resident images (bnhip_png_encode_device), by HIP events around the five launches.
Reported beside the times: the bytes each form returns over PCIe, and stream / raw beside zlib-6 / raw on the same images (raw: the
filtered bytes H (W + 1) per image).  (b)'s streams are decoded and compared with (a)'s indices.
The library is the one host.py loads: BNHIP_LIB names another build, so --legs g (bnhip_spectrogram_pcm16 alone, the guard) run
against the parent commit's library gives the other side of the uniform guard.  Host clock around calls that end in a synchronise;
--warmup warm-up and --reps timed repetitions per leg, the legs alternated twice.  Prints one JSON line and writes it to --out.

    python tools/png_rate.py [--legs abcg] [--reps 20] [--warmup 3] [--out profiles/r17_png_rate.json]
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import birdnet_go_amd  # noqa: E402,F401
from birdnet_go_amd import host, spectrogram as sg  # noqa: E402
from spectrogram_rate import clips_48k  # noqa: E402


def host_png(img, pal):
    """spectrogram.write_png's bytes, in memory."""
    h, w = img.shape
    rows = np.zeros((h, w + 1), np.uint8)
    rows[:, 1:] = img
    c = sg._chunk
    return (b"\x89PNG\r\n\x1a\n" + c(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 3, 0, 0, 0)) + c(b"PLTE", pal.tobytes())
            + c(b"IDAT", zlib.compress(rows.tobytes(), 6)) + c(b"IEND", b""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=int, default=15)
    ap.add_argument("--size", default="lg")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="abcg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_png_rate.json"))
    a = ap.parse_args()
    host.init()                                                      # no device: a loud error, not a fallback
    rate, prof = 48000, sg.bird_profile()
    width = sg.size_to_pixels(a.size)
    height, _ = host.spectrogram_size(width)
    pal = sg.palette("default")
    pcm = clips_48k(a.clips, a.seconds, rate)
    B = a.clips
    raw = B * height * (width + 1)
    with open(host.LIB_PATH, "rb") as fh:
        digest = hashlib.sha256(fh.read()).hexdigest()[:16]
    res = {"tool": "png_rate", "library": os.path.relpath(host.LIB_PATH, ROOT), "library_sha256_16": digest, "clips": B, "seconds": a.seconds,
           "rate_in": rate, "rate_out": prof.resample_rate, "width": width, "height": height, "reps": a.reps, "warmup": a.warmup,
           "pcm_bytes": int(pcm.nbytes), "raw_filtered_bytes": raw}
    render = lambda: host.spectrogram(pcm, rate, width, rate_out=prof.resample_rate)
    legs = {"g": render,
            "a": lambda: [host_png(im, pal) for im in render()],
            "b": lambda: host.spectrogram_png(pcm, rate, width, pal, rate_out=prof.resample_rate, raw=True)}
    blocks = []
    if "c" in a.legs:
        hip = C.CDLL("libamdhip64.so")                               # device memory through the HIP runtime the library itself uses
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        hip.hipEventSynchronize.argtypes = [C.c_void_p]
        hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]

        def dev(nbytes):
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), nbytes) == 0
            blocks.append(p)
            return p
        img = render()
        cap, ws = host.png_max_bytes(B, width, height), host.png_workspace_size(B, width, height)
        d_in, d_out, d_off, d_ws = dev(img.nbytes), dev(cap), dev(8 * (B + 1)), dev(ws)
        assert hip.hipMemcpy(d_in, img.ctypes.data, img.nbytes, 1) == 0
        e0, e1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0

        def leg_c():
            assert hip.hipEventRecord(e0, None) == 0
            host.png_encode_device(d_in, B, width, height, pal, d_out, cap, d_off, d_ws, ws)
            assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
            ms = C.c_float(0)
            assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
            return ms.value
        legs["c"] = leg_c
    run = [l for l in "gabc" if l in a.legs]
    ts, got = {l: [] for l in run}, {}
    for l in run:
        for _ in range(a.warmup):
            legs[l]()
    for p in range(2):                                               # the legs alternated twice
        for l in run:
            for _ in range(a.reps // 2):
                t0 = time.perf_counter()
                got[l] = legs[l]()
                ts[l].append(got[l] if l == "c" else (time.perf_counter() - t0) * 1e3)
    names = {"g": "g_spectrogram_pcm16", "a": "a_render_then_host_zlib6", "b": "b_spectrogram_png_one_call", "c": "c_png_kernels_by_events"}
    for l in run:
        v = np.array(ts[l])
        res[names[l] + "_ms"] = round(float(np.median(v)), 3)
        res[names[l] + "_min_ms"] = round(float(v.min()), 3)
        res[names[l] + "_pass_medians_ms"] = [round(float(np.median(h)), 3) for h in np.split(v, 2)]
    ok = True
    if "a" in run:
        zb = sum(len(s) for s in got["a"])
        res["a_bytes_over_pcie_d2h"] = int(B * height * width)
        res["a_png_bytes"] = zb
        res["zlib6_over_raw"] = round(zb / raw, 4)
        if "g" in run:
            res["a_host_zlib6_alone_ms"] = round(res[names["a"] + "_ms"] - res[names["g"] + "_ms"], 3)
    if "b" in run:
        out, off = got["b"]
        res["b_bytes_over_pcie_d2h"] = int(off[-1]) + 8 * (B + 1)
        res["b_png_bytes"] = int(off[-1])
        res["stream_over_raw"] = round(int(off[-1]) / raw, 4)
        img = render()
        same = all(np.array_equal(sg.read_png_indices(out[int(off[i]):int(off[i + 1])].tobytes()), img[i]) for i in range(B))
        res["b_decodes_to_the_rendered_indices"] = bool(same)
        ok = ok and same
        if "a" in run:
            res["speedup_b_over_a"] = round(res[names["a"] + "_ms"] / res[names["b"] + "_ms"], 2)
            res["d2h_bytes_b_over_a"] = round(res["b_bytes_over_pcie_d2h"] / res["a_bytes_over_pcie_d2h"], 4)
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
