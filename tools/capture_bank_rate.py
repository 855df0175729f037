"""The capture bank at the size of a 256-source station ("Capture bank"), one mode per process:

  --mode write    one tick's bnhip_capture_bank_write of --sources sources x 1.5 s of 48 kHz int16: p50 / p95 / min over --calls calls
                  after two warm-ups, host clock around the call (it ends in its synchronise).
  --mode export   --clips due clips of 15 s out of --sources rings of --seconds s: bnhip_capture_bank_clips against the two-call host
                  form on the same library - a numpy cut out of the host's own rings, then bnhip_loudness_flac_ragged_pcm16 and
                  bnhip_loudness_ragged_normalize_pcm16 + bnhip_spectrogram_png_ragged_pcm16 with the PCM uploaded.  The legs alternate in
                  --rounds rounds; the bytes must be equal (asserted); the PCIe bytes of each leg are counted from the calls' layouts.
  --mode cut      --calls bnhip_capture_bank_read_pcm16 calls of 256 spans of 15 s and nothing else: the process for a kernel trace, whose
                  k_ring_cut rows are the kernel's time.  BNHIP_RING_CUT=element runs the element-load form of the same kernel.
  --mode filecut  the same burst through bnhip_recording_clips_pcm16 (k_cut_clips<16>), for the same trace.
  --mode writes   --calls write calls and nothing else, for the trace's k_capture_write rows.
Prints one JSON line.

    python tools/capture_bank_rate.py --mode write|export|cut|filecut|writes [--sources 256] [--seconds 120] [--clips 64] [--calls 40]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import birdnet_go_amd  # noqa: E402,F401
from birdnet_go_amd import host, spectrogram  # noqa: E402

RATE = 48000


def stats(ts):
    ts = np.asarray(ts)
    return {"p50_ms": round(float(np.percentile(ts, 50)), 3), "p95_ms": round(float(np.percentile(ts, 95)), 3), "min_ms": round(float(ts.min()), 3),
            "max_ms": round(float(ts.max()), 3), "n": int(ts.size)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def tick_frames(rng, n_src, n):
    base = (np.clip(rng.normal(0, 0.1, n + n_src), -1, 1) * 32767).astype("<i2")
    return [(s, base[s:s + n].tobytes()) for s in range(n_src)]


def spans_of(n, n_src, length, written):
    q = np.zeros(n, host.CLIP_SPAN)
    for i in range(n):
        q[i] = (written - length - 150 * i, length, (i * 7) % n_src)
    return q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", required=True, choices=["write", "export", "cut", "filecut", "writes"])
    ap.add_argument("--sources", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    host.init()                                                          # no device: a loud error, not a fallback
    rng = np.random.default_rng(1)
    out = {"mode": a.mode, "sources": a.sources}
    clip = 15 * RATE
    if a.mode == "filecut":
        n = 16 * RATE
        rec = (np.clip(rng.normal(0, 0.1, n), -1, 1) * 32767).astype("<i2")
        raw = np.tile(rec, 256).tobytes()
        table = host.channel_recordings([n] * 256, RATE, 16, 1, 0)
        q = np.zeros(256, host.CLIP_SPAN)
        for i in range(256):
            q[i] = (n - clip - 3 * i, clip, i)
        ts = [timed(lambda: host.recording_clips(raw, table, RATE, q))[1] for _ in range(a.calls)]
        out.update(call=stats(ts), clip_samples=clip, clips=256)
        print(json.dumps(out))
        return
    seconds = a.seconds if a.mode == "export" else 16.0
    bank = host.CaptureBank(a.sources, seconds, RATE)
    out.update(capacity_samples=bank.capacity, ring_bytes=a.sources * bank.capacity * 2)
    tick = int(1.5 * RATE)
    if a.mode in ("write", "writes"):
        frames = tick_frames(rng, a.sources, tick)
        for _ in range(2):
            bank.write(frames)
        ts = [timed(lambda: bank.write(frames))[1] for _ in range(a.calls)]
        out.update(call=stats(ts), bytes_per_call=a.sources * tick * 2)
    elif a.mode == "cut":
        for _ in range(12):
            bank.write(tick_frames(rng, a.sources, tick))
        q = spans_of(256, a.sources, clip, int(bank.positions()[0][0]))
        ts = [timed(lambda: bank.read(q))[1] for _ in range(a.calls)]
        out.update(call=stats(ts), clip_samples=clip, clips=256, form=os.environ.get("BNHIP_RING_CUT", "default"))
    else:
        # the host's own rings beside the device's, fed the same bytes: what a host keeps today
        mine = np.zeros((a.sources, bank.capacity), np.int16)
        written = 0
        for _ in range(int(np.ceil(20 * RATE / tick))):                  # 20 s of audio: every clip lies in what was written
            frames = tick_frames(rng, a.sources, tick)
            bank.write(frames)
            for s, f in frames:
                x = np.frombuffer(f, "<i2")
                mine[s, (written + np.arange(x.size)) % bank.capacity] = x
            written += tick
        q = spans_of(a.clips, a.sources, clip, written)
        x = host.ClipSettings(1, 1, 1, False, True, lpc_order=8, width=400, palette=spectrogram.palette())
        pal = spectrogram.palette()

        def fused():
            return bank.export_raw(q, x)

        def composed():
            clips = [mine[int(s["recording"]), (int(s["start"]) + np.arange(int(s["length"]))) % bank.capacity] for s in q]
            loud, fl = host.loudness_flac_ragged(clips, RATE, lpc_order=8)
            gained = host.loudness_normalize_ragged(clips, RATE)[1]
            return loud, fl, host.spectrogram_png_ragged(gained, RATE, 400, pal)

        fused(), composed()                                               # warm-up
        legs = {"fused": [], "composed": []}
        for _ in range(a.rounds):
            g, t = timed(fused)
            legs["fused"].append(t)
            (loud, fl, png), t = timed(composed)
            legs["composed"].append(t)
            assert g.n_clips == a.clips and g.flac == fl and g.png == png and [bytes(r) for r in g.loudness] == [bytes(r) for r in loud]
        pcm = int(q["length"].sum()) * 2
        streams = sum(len(s) for s in g.flac) + sum(len(s) for s in g.png)
        out.update(fused=stats(legs["fused"]), composed=stats(legs["composed"]), clips=a.clips, bytes_equal=True,
                   pcie_bytes={"fused": {"up": int(q.nbytes), "down": streams},
                               "composed": {"up": 3 * pcm, "down": streams + pcm, "note": "the clips go up three times (FLAC, normalise, render) and the gained PCM comes back once"}})
    bank.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
