"""Detection clips of one long recording on the full synthetic model, two ways (DESIGN section 9 "File analysis: detection clips"):
  (a) one bnhip_analyze_channels_pcm_clips call: the events, and behind them the cut, the normalise, the FLAC encode, the render and
      the PNG encode on the recordings where they lie;
  (b) what a host does without it: bnhip_analyze_channels_pcm_events, the span rule, a cut of its own copy of the recording, then
      bnhip_loudness_flac_ragged_pcm16, and for the images bnhip_loudness_ragged_normalize_pcm16 (the gained PCM) and
      bnhip_spectrogram_png_ragged_pcm16 - the clips cross to the device again in each of the three.
The same for the recording as a stereo file (both channels the same material, channel 0 read): (a) takes the interleaved frames,
(b) de-interleaves on the host first.  The legs run in one process, alternated round by round, host clock around calls that end in a
synchronise; medians over --rounds after one warm-up of each, [min, max] beside them.  (a) must equal (b): events, spans, FLAC and PNG
bytes, asserted.  The filter's thresholds come from the rows of a warm-up call (tools/analyze_events_rate.py).  Prints one JSON line.

    python tools/analyze_clips_rate.py [--seconds 3600] [--overlap 2.5] [--rounds 3] [--max-batch 256] [--max-clips 256]
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
from birdnet_go_amd import host, spectrogram, synth_model as sm, wav  # noqa: E402
from analyze_events_rate import filter_from, stats, timed  # noqa: E402
from analyze_rate import CLIP, RATE, recording  # noqa: E402

WIDTH = 400


def legs(c, pcm, channels, hop, min_tail, k, overlap, rounds, max_clips):
    mono_table = host.channel_recordings([pcm.size], RATE, 16, 1, 0)
    table = host.channel_recordings([pcm.size], RATE, 16, channels, 0)
    frames = pcm if channels == 1 else np.ascontiguousarray(np.repeat(pcm[:, None], channels, axis=1)).reshape(-1)
    rows = c.analyze_channels_pcm(pcm, mono_table, RATE, hop, min_tail, k=k, threshold=float("-inf"))[0]
    f = filter_from(rows, c.num_species(), hop, overlap)
    flt = host.EventTables(f.class_threshold, f.class_veto, f.veto_threshold, f.hold_windows, f.min_count, 0)
    pal = spectrogram.palette()
    x = host.ClipSettings(3 * RATE, 12 * RATE, 2 ** 31 - 1, lpc_order=8, seek_interval=RATE, width=WIDTH, rate_out=24000, palette=pal)
    parts = {"deinterleave": [], "events_call": [], "host_cut": [], "loudness_flac": [], "normalize": [], "spectrogram_png": []}

    def a():
        return c.analyze_channels_pcm_clips(frames, table, RATE, hop, flt, x, min_tail, k=k, max_clips=max_clips)

    def b(keep=None):
        mono, t0 = timed(lambda: frames if channels == 1 else np.ascontiguousarray(frames.reshape(-1, channels)[:, 0]))
        (ev, _), t1 = timed(lambda: c.analyze_channels_pcm_events(mono, mono_table, RATE, hop, flt, min_tail, k=k))
        (spans, clips), t2 = timed(lambda: _cut(mono, ev, hop, x, max_clips))
        (loud, flac), t3 = timed(lambda: host.loudness_flac_ragged(clips, RATE, seek_interval=RATE, lpc_order=8))
        gained, t4 = timed(lambda: host.loudness_normalize_ragged(clips, RATE)[1])
        png, t5 = timed(lambda: host.spectrogram_png_ragged(gained, RATE, WIDTH, pal, rate_out=24000))
        if keep is not None:
            for name, t in zip(parts, (t0, t1, t2, t3, t4, t5)):
                keep[name].append(t)
        return ev, spans, loud, flac, png

    got, want = a(), b()                                                 # warm-up of both, and the comparison
    n = got.n_clips
    same = bool(np.array_equal(got.events, want[0]) and np.array_equal(got.spans, want[1]) and got.flac == want[3][:n] and got.png == want[4][:n]
                and [bytes(r) for r in got.loudness] == [bytes(r) for r in want[2][:n]] and n == len(want[3]))
    ts = {"a_fused_call": [], "b_events_then_host_clips": []}
    for _ in range(rounds):
        ts["a_fused_call"].append(timed(a)[1])
        ts["b_events_then_host_clips"].append(timed(lambda: b(parts))[1])
    r = {"channels": channels, "hop": hop, "events": int(got.n_events), "clips": int(n), "clip_samples": int(sum(int(s) for s in got.spans["length"][:n])),
         "flac_bytes": int(sum(len(s) for s in got.flac)), "png_bytes": int(sum(len(s) for s in got.png)), "a_equals_b": same}
    r.update({name: stats(t) for name, t in ts.items()})
    r["b_parts"] = {name: stats(t) for name, t in parts.items()}
    return r, same


def _cut(mono, ev, hop, x, max_clips):
    spans = host.event_clip_spans(ev, [mono.size], hop, x)
    clips = [mono[int(s["start"]):int(s["start"]) + int(s["length"])] for s in spans if int(s["length"]) > 0][:max_clips]
    return spans, clips


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=3600)
    ap.add_argument("--overlap", type=float, default=2.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--max-clips", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--channels", default="1,2")
    a = ap.parse_args()
    host.init()                                                          # no device: a loud error, not a fallback
    c = host.HipClassifier(sm.build_model(sm.SynthConfig()), max_batch=a.max_batch)
    pcm = recording(a.seconds)
    _, clip_len, hop, min_tail = wav.window_table([pcm.size], RATE, 3.0, a.overlap)
    assert clip_len == CLIP
    res = {"tool": "analyze_clips_rate", "seconds": a.seconds, "rate": RATE, "bits": 16, "overlap": a.overlap, "max_batch": a.max_batch,
           "rounds": a.rounds, "k": a.k, "max_clips": a.max_clips, "image": [WIDTH, host.spectrogram_size(WIDTH)[0]], "legs": {}}
    ok = True
    for ch in [int(v) for v in a.channels.split(",")]:
        r, same = legs(c, pcm, ch, hop, min_tail, a.k, a.overlap, a.rounds, a.max_clips)
        ok = ok and same
        res["legs"]["mono" if ch == 1 else f"{ch}ch"] = r
        print(json.dumps(r), file=sys.stderr, flush=True)
    c.close()
    res["a_equals_b"] = ok
    print(json.dumps(res))
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
