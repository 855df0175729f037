"""File analysis of one long recording on the full synthetic model, two ways (DESIGN section 9 "File analysis"):
  (dev)  one bnhip_analyze_pcm_topk call: the recording's int16 samples go to the device once and the windows are framed there;
  (host) the host-framed path: every overlapping window materialised in numpy by wav.frame_clips' rule (as int16, the cheaper of
         the host's options: 2 bytes a sample, not frame_clips' float32), then one bnhip_predict_pcm_topk call over them.
Both legs run in one process, alternated round by round, host clock around calls that end in a synchronise; medians over --rounds
after one warm-up of each.  The device-framed result is compared bit for bit with bnhip_predict_pcm_topk of the host-framed windows sent
in calls of 96 - the engine's unsplit route, which the device-framed chunks take too; a host call of 128 clips or more goes through
the host pipeline, whose chunks run the full-batch tile shapes and differ from the unsplit route in the last bits whatever the
input's origin (max_abs_conf_vs_pipelined_call records that distance; the top-k indices must agree).  copy_share: a plain hipMemcpy of the recording's bytes from
the same pageable array, timed alone, over the device-framed call's time.  Prints one JSON line.

    python tools/analyze_rate.py [--seconds 3600] [--overlaps 0,1.5,2.0,2.5] [--rounds 3] [--max-batch 256]
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
import birdnet_go_amd  # noqa: E402,F401
from birdnet_go_amd import host, synth_model as sm, wav  # noqa: E402

RATE, CLIP = 48000, 144000


def recording(seconds):
    """int16 material: a minute of synthetic clips, repeated with a slow level change so that no two windows are equal."""
    minute = sm.synth_clips(20, CLIP, RATE).reshape(-1)
    minute = minute / np.abs(minute).max()
    n = seconds * RATE
    reps = (n + minute.size - 1) // minute.size
    level = np.repeat(np.linspace(0.3, 0.9, reps, dtype=np.float32), minute.size)[:n]
    return np.round(np.tile(minute, reps)[:n] * level * 30000.0).astype(np.int16)


def host_windows(pcm, hop, min_tail):
    first = host.analyze_windows([pcm.size], CLIP, hop, min_tail)
    w = int(first[-1])
    out = np.zeros((w, CLIP), np.int16)
    whole = min(w, (pcm.size - CLIP) // hop + 1)
    out[:whole] = np.lib.stride_tricks.as_strided(pcm, (whole, CLIP), (hop * 2, 2))
    for j in range(whole, w):                                       # the zero-padded tail window
        seg = pcm[j * hop:]
        out[j, :seg.size] = seg
    return out


def copy_ms(pcm, rounds):
    hip = C.CDLL("libamdhip64.so")
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(pcm.nbytes)) == 0
    ts = []
    for _ in range(rounds + 1):
        t0 = time.perf_counter()
        assert hip.hipMemcpy(p, pcm.ctypes.data_as(C.c_void_p), C.c_size_t(pcm.nbytes), 1) == 0
        assert hip.hipDeviceSynchronize() == 0
        ts.append((time.perf_counter() - t0) * 1e3)
    hip.hipFree(p)
    return float(np.median(ts[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--overlaps", default="0,1.5,2.0,2.5")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    a = ap.parse_args()
    host.init()                                                      # no device: a loud error, not a fallback
    pcm = recording(a.seconds)
    c = host.HipClassifier(sm.build_model(sm.SynthConfig()), max_batch=a.max_batch)
    res = {"tool": "analyze_rate", "seconds": a.seconds, "rate": RATE, "bits": 16, "max_batch": a.max_batch, "rounds": a.rounds,
           "recording_bytes": int(pcm.nbytes), "overlaps": {}}
    res["h2d_recording_copy_ms"] = round(copy_ms(pcm, a.rounds), 2)
    ok = True
    for ov in [float(v) for v in a.overlaps.split(",")]:
        _, clip_len, hop, min_tail = wav.window_table([pcm.size], RATE, 3.0, ov)
        assert clip_len == CLIP

        def dev():
            return c.analyze_pcm_topk(pcm, 16, [pcm.size], hop, min_tail, k=a.k)[:2]

        def hst():
            w = host_windows(pcm, hop, min_tail)
            return c.predict_pcm_topk(w.reshape(-1), 16, w.shape[0], k=a.k)

        got, piped = dev(), hst()                                    # warm-up of both legs, and the comparison
        w = host_windows(pcm, hop, min_tail)
        parts = [c.predict_pcm_topk(w[i:i + 96].reshape(-1), 16, min(96, w.shape[0] - i), k=a.k) for i in range(0, w.shape[0], 96)]
        want = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        del w, parts
        same = bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]))
        ok = ok and same and bool(np.array_equal(got[1], piped[1]))
        td, th = [], []
        for _ in range(a.rounds):
            for fn, ts in ((dev, td), (hst, th)):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
        w = got[0].shape[0]
        d, h = float(np.median(td)), float(np.median(th))
        r = {"hop": hop, "windows": w, "device_framed_ms": round(d, 1), "host_framed_ms": round(h, 1), "device_framed_all_ms": [round(t, 1) for t in td],
             "host_framed_all_ms": [round(t, 1) for t in th], "speedup": round(h / d, 2), "device_framed_windows_per_s": round(w / (d / 1e3)),
             "host_framed_windows_per_s": round(w / (h / 1e3)), "copy_share": round(res["h2d_recording_copy_ms"] / d, 3),
             "host_bytes_sent": int(w) * CLIP * 2, "bit_identical": same,
             "max_abs_conf_vs_pipelined_call": float(np.abs(got[0] - piped[0]).max()), "idx_equal_pipelined_call": bool(np.array_equal(got[1], piped[1]))}
        res["overlaps"][str(ov)] = r
        print(json.dumps({str(ov): r}), file=sys.stderr, flush=True)
    c.close()
    res["bit_identical"] = ok
    print(json.dumps(res))
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
