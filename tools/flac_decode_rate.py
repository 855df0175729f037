"""Cost of reading saved FLAC clips back on the device ("FLAC decode"): the README's burst - 64 clips at 48 kHz with
64 distinct lengths between 9 s and 45 s (tools/ragged_rate.py's burst, seed 16, material from tools/spectrogram_rate.py's generator)
- encoded by the device encoder at lpc_order 8, then:
  (d) bnhip_flac_decode_pcm16, the whole burst in one call: streams up, PCM back;
  (k) the decoder's kernels alone on device-resident streams through bnhip_flac_decode_device, by HIP events;
  (f) bnhip_flac_spectrogram_png: decode, render (bird profile, resampled to 24 kHz on the device, "lg": 1026 x 513) and PNG-encode in
      one call, the compressed streams going up;
  (p) bnhip_spectrogram_png_ragged_pcm16 on the same clips' PCM: the same images, the PCM going up.
The entries are called through ctypes on buffers prepared once, so a leg times the C call and not the Python wrapper's packing.  Host
clock around calls that end in a synchronise; --warmup warm-up and --reps timed repetitions per leg, the legs alternated twice.  (d)
is checked against the clips in every sample, (f) against (p) in every byte.  No native host FLAC decoder is on the build machine to
stand beside (d), and the Python one of tests/ is not a yardstick, so there is no host leg.  Prints one JSON line and writes it to
--out.

    python tools/flac_decode_rate.py [--legs dkfp] [--reps 20] [--warmup 3] [--seed 16] [--out profiles/r19_flac_decode_rate.json]
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
from birdnet_go_amd import flac, host, spectrogram as sg  # noqa: E402
from ragged_rate import burst_lengths  # noqa: E402
from spectrogram_rate import clips_48k  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--size", default="lg")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="dkfp")
    ap.add_argument("--seed", type=int, default=16)
    ap.add_argument("--lpc-order", type=int, default=flac.LEVEL5_LPC_ORDER)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_flac_decode_rate.json"))
    a = ap.parse_args()
    host.init()                                                      # no device: a loud error, not a fallback
    lib = host.load_library()
    rate, rate_out = 48000, sg.bird_profile().resample_rate
    width = sg.size_to_pixels(a.size)
    height, fft = host.spectrogram_size(width)
    pal = host._png_palette(sg.palette("default"))
    lens = burst_lengths(a.clips, rate, a.seed)
    long_clips = clips_48k(a.clips, 45, rate)
    burst = [np.ascontiguousarray(long_clips[i, :n]) for i, n in enumerate(lens)]
    del long_clips
    streams = flac.encode_clips(burst, rate, lpc_order=a.lpc_order, ragged=True, seek_interval=rate)
    buf, offsets = host._flac_burst(streams)
    packed, lens32 = host.ragged_pack(burst)
    n, total = a.clips, int(packed.size)
    infos = [host.flac_stream_info(s) for s in streams]
    with open(host.LIB_PATH, "rb") as fh:
        digest = hashlib.sha256(fh.read()).hexdigest()[:16]
    res = {"tool": "flac_decode_rate", "library": os.path.relpath(host.LIB_PATH, ROOT), "library_sha256_16": digest, "clips": n, "rate": rate,
           "rate_out": rate_out, "seed": a.seed, "lpc_order": a.lpc_order, "lengths": lens, "pcm_bytes": 2 * total,
           "flac_bytes": int(offsets[-1]), "flac_over_pcm": round(float(offsets[-1]) / (2 * total), 4),
           "frames": int(sum((v + 4095) // 4096 for v in lens)), "width": width, "height": height, "fft_size": fft, "reps": a.reps,
           "warmup": a.warmup, "host_decoder_leg": "none: no native host FLAC decoder on the build machine"}
    vp, ci, sz, cd = C.c_void_p, C.c_int, C.c_size_t, C.c_double
    pcm_out, lens_out, results = np.empty(total, np.int16), np.zeros(n, np.int32), (host.FlacDecodeResult * n)()
    cap = host.png_max_bytes(n, width, height)
    png_f, off_f = np.empty(cap, np.uint8), np.zeros(n + 1, np.uint64)
    png_p, off_p = np.empty(cap, np.uint8), np.zeros(n + 1, np.uint64)
    lib.bnhip_flac_decode_pcm16.argtypes = [ci, vp, ci, vp, vp, sz, vp, vp]
    lib.bnhip_flac_spectrogram_png.argtypes = [ci, vp, ci, vp, ci, ci, ci, vp, cd, cd, vp, vp, sz, vp, vp]
    lib.bnhip_spectrogram_png_ragged_pcm16.argtypes = [ci, vp, ci, vp, ci, ci, ci, ci, vp, cd, cd, vp, vp, sz, vp]

    def check(rc):
        if rc != host.BNHIP_OK:
            raise SystemExit(f"entry failed: {rc} {lib.bnhip_last_error()}")

    legs = {
        "d": lambda: check(lib.bnhip_flac_decode_pcm16(0, buf.ctypes.data, n, offsets.ctypes.data, pcm_out.ctypes.data, total, lens_out.ctypes.data,
                                                       C.addressof(results))),
        "f": lambda: check(lib.bnhip_flac_spectrogram_png(0, buf.ctypes.data, n, offsets.ctypes.data, rate_out, width, height, None, 0.0, 100.0,
                                                          pal.ctypes.data, png_f.ctypes.data, cap, off_f.ctypes.data, C.addressof(results))),
        "p": lambda: check(lib.bnhip_spectrogram_png_ragged_pcm16(0, packed.ctypes.data, n, lens32.ctypes.data, rate, rate_out, width, height, None,
                                                                  0.0, 100.0, pal.ctypes.data, png_p.ctypes.data, cap, off_p.ctypes.data)),
    }
    lib.bnhip_last_error.restype = C.c_char_p
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

        ws = host.flac_decode_workspace_size(infos, offsets)
        res["workspace_bytes"] = ws
        d_in, d_pcm, d_res, d_ws = dev(buf.nbytes, buf), dev(2 * total), dev(16 * n), dev(ws)

        def kernels():
            assert hip.hipEventRecord(e0, None) == 0
            host.flac_decode_device(d_in, offsets, infos, d_pcm, total, d_res, d_ws, ws)
            assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
            ms = C.c_float(0.0)
            assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
            return ms.value
        events["k"] = kernels
    run = [l for l in "dkfp" if l in a.legs]
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
    names = {"d": "d_decode_pcm16_one_call", "k": "k_decode_kernels_events", "f": "f_flac_to_png_one_call", "p": "p_pcm_to_png_one_call"}
    for l in run:
        v = np.array(ts[l])
        res[names[l] + "_ms"] = round(float(np.median(v)), 3)
        res[names[l] + "_min_ms"] = round(float(v.min()), 3)
        res[names[l] + "_pass_medians_ms"] = [round(float(np.median(h)), 3) for h in np.split(v, 2)]
    ok = True
    if "d" in run:
        res["d_equals_clips"] = bool(np.array_equal(pcm_out, packed) and lens_out.tolist() == list(lens) and all(r.status == host.FLAC_OK for r in results))
        res["d_decoded_pcm_gb_per_s"] = round(2 * total / res["d_decode_pcm16_one_call_ms"] / 1e6, 3)
        ok = ok and res["d_equals_clips"]
    if "k" in run:
        got = np.empty(total, np.int16)
        assert hip.hipMemcpy(got.ctypes.data, d_pcm, got.nbytes, 2) == 0
        res["k_equals_clips"] = bool(np.array_equal(got, packed))
        res["k_decoded_pcm_gb_per_s"] = round(2 * total / res["k_decode_kernels_events_ms"] / 1e6, 3)
        ok = ok and res["k_equals_clips"]
    if "d" in run and "k" in run:
        res["k_kernel_share_of_d"] = round(res["k_decode_kernels_events_ms"] / res["d_decode_pcm16_one_call_ms"], 3)
    if "f" in run and "p" in run:
        res["png_bytes"] = int(off_p[-1])
        res["f_equals_p"] = bool(off_f.tolist() == off_p.tolist() and np.array_equal(png_f[:int(off_f[-1])], png_p[:int(off_p[-1])]))
        res["f_over_p"] = round(res["f_flac_to_png_one_call_ms"] / res["p_pcm_to_png_one_call_ms"], 3)
        ok = ok and res["f_equals_p"]
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
