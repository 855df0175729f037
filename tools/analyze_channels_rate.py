"""File analysis of a stereo recording on the full synthetic model (DESIGN section 9 "File analysis", multichannel): an hour of
stereo 48 kHz int16, as a field recorder writes it -
  (a) one bnhip_analyze_channels_pcm_topk call: the interleaved frames go to the device as they are in the file and the slot launch
      fetches the channel - with a fixed channel, with the mix, and with auto (the energy measurement in front of the slot launch);
  (b) today's path: wav._first_channel's de-interleaving pass on the host (numpy, one thread), then bnhip_analyze_pcm_topk over the
      int16 channel.  Reported with and without the host pass;
  (c) the floor: the same audio as a mono file through bnhip_analyze_pcm_topk.
The legs run in one process, alternated round by round, host clock around calls that end in a synchronise; medians over --rounds
after one warm-up of each, every round's time kept.  (a) with the fixed channel must equal (b) bit for bit: the tool's one hard
assertion.  The two new launches are reported as differences of legs that share everything else: auto - fixed is the measurement
(two launches), fixed - (b without its host pass) is the second channel's bytes over PCIe plus the slot launch against the framed
launch reading int16 where it lies; bnhip_channel_energy_pcm alone (upload, measurement, 48 bytes down) is timed too.  The library
is the one host.py loads: BNHIP_LIB names another build, so `--legs bc` against the parent commit's library gives (b) and (c) as
they were before this entry existed.  Prints one JSON line and, with --out, writes it there.

    python tools/analyze_channels_rate.py [--minutes 60] [--overlap 0] [--rounds 3] [--max-batch 256] [--legs abc] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import birdnet_go_amd  # noqa: E402,F401
from birdnet_go_amd import host, synth_model as sm, wav  # noqa: E402

MODEL_RATE, CLIP = 48000, 144000


def stereo(seconds, seed=3):
    """int16 frames [n, 2]: a minute of tones and noise per channel, repeated with a level of its own per minute; the left channel
    about 9 dB above the right one, so auto picks it."""
    rng = np.random.default_rng(seed)
    n = 60 * MODEL_RATE
    t = np.arange(n, dtype=np.float32) / np.float32(MODEL_RATE)
    minute = np.zeros((n, 2), np.float32)
    for ch, gain in ((0, 1.0), (1, 0.35)):
        for f in (440.0 + 300.0 * ch, 2100.0 + 500.0 * ch, 6300.0):
            minute[:, ch] += np.sin(np.float32(2 * np.pi * f) * t)
        minute[:, ch] = (minute[:, ch] / 3.2 + 0.05 * rng.standard_normal(n).astype(np.float32)) * np.float32(gain)
    reps = (seconds + 59) // 60
    out = np.empty((reps * n, 2), np.int16)
    for i, level in enumerate(np.linspace(0.3, 0.9, reps)):
        out[i * n:(i + 1) * n] = np.round(minute * np.float32(level * 30000.0)).clip(-32768, 32767).astype(np.int16)
    return out[:seconds * MODEL_RATE]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=int, default=60)
    ap.add_argument("--overlap", type=float, default=0.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    host.init()                                                      # no device: a loud error, not a fallback
    seconds = a.minutes * 60
    frames = stereo(seconds)
    n = frames.shape[0]
    raw = frames.reshape(-1).view(np.uint8)
    as_file = frames.view(np.uint8).reshape(n, 2, 2)                 # what wav._first_channel slices: [frame, channel, byte]
    mono = np.ascontiguousarray(frames[:, 0])
    _, clip_len, hop, min_tail = wav.window_table([CLIP], MODEL_RATE, 3.0, a.overlap)
    assert clip_len == CLIP
    c = host.HipClassifier(sm.build_model(sm.SynthConfig()), max_batch=a.max_batch)
    with open(host.LIB_PATH, "rb") as fh:
        digest = hashlib.sha256(fh.read()).hexdigest()[:16]
    res = {"tool": "analyze_channels_rate", "library": os.path.relpath(host.LIB_PATH, ROOT), "library_sha256_16": digest, "legs": a.legs,
           "minutes": a.minutes, "rate": MODEL_RATE, "bits": 16, "channels": 2, "frames": int(n), "hop": int(hop), "max_batch": a.max_batch,
           "rounds": a.rounds, "pcie_bytes": {"a": int(raw.size), "b": int(mono.nbytes), "c": int(mono.nbytes)}}
    t_host = []
    chosen = {}

    def leg_a(select):
        def run():
            conf, idx, _, sel = c.analyze_channels_pcm_topk(raw, host.channel_recordings([n], MODEL_RATE, 16, 2, select), MODEL_RATE, hop, min_tail, k=a.k)
            chosen[str(select)] = int(sel[0])
            return conf, idx
        return run

    def leg_b():
        t0 = time.perf_counter()
        first = np.ascontiguousarray(as_file[:, 0, :]).tobytes()     # wav.read_wav_pcm: the first channel's bytes
        t_host.append((time.perf_counter() - t0) * 1e3)
        return c.analyze_pcm_topk(first, 16, [n], hop, min_tail, k=a.k)[:2]

    def leg_c():
        return c.analyze_pcm_topk(mono, 16, [n], hop, min_tail, k=a.k)[:2]

    def leg_e():
        return host.channel_energy(raw, host.channel_recordings([n], MODEL_RATE, 16, 2, 0))

    legs = []
    if "a" in a.legs:
        legs += [("a_fixed", leg_a(0)), ("a_mix", leg_a("mix")), ("a_auto", leg_a("auto")), ("energy_entry", leg_e)]
    if "b" in a.legs:
        legs.append(("b", leg_b))
    if "c" in a.legs:
        legs.append(("c", leg_c))
    first = {name: f() for name, f in legs}                           # warm-up of every leg, and the comparisons
    same = None
    if "a_fixed" in first and "b" in first:
        same = bool(np.array_equal(first["a_fixed"][0], first["b"][0]) and np.array_equal(first["a_fixed"][1], first["b"][1]))
        res["bit_identical_a_fixed_b"] = same
        # auto picks the louder left channel here, so its rows are the fixed call's
        res["bit_identical_a_auto_a_fixed"] = bool(np.array_equal(first["a_auto"][0], first["a_fixed"][0]) and
                                                   np.array_equal(first["a_auto"][1], first["a_fixed"][1]))
        res["chosen"] = dict(chosen)
        res["rms_dbfs"] = [round(float(v), 3) for v in first["energy_entry"][0]["rms_dbfs"]]
    t_host.clear()
    ts = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, f in legs:
            t0 = time.perf_counter()
            f()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    res["windows"] = int(next(v for k, v in first.items() if k != "energy_entry")[0].shape[0])
    for name in ts:
        res[name + "_ms"] = round(float(np.median(ts[name])), 1)
        res[name + "_all_ms"] = [round(t, 1) for t in ts[name]]
    if "b" in ts:
        res["b_host_pass_ms"] = round(float(np.median(t_host)), 1)
        res["b_without_host_pass_ms"] = round(float(np.median([t - v for t, v in zip(ts["b"], t_host)])), 1)
    if "a_fixed" in ts:
        res["energy_launches_ms_auto_minus_fixed"] = round(res["a_auto_ms"] - res["a_fixed_ms"], 1)
    if "a_fixed" in ts and "b" in ts:
        res["second_channel_and_slot_launch_ms_fixed_minus_b_device"] = round(res["a_fixed_ms"] - res["b_without_host_pass_ms"], 1)
        res["speedup_a_fixed_over_b"] = round(res["b_ms"] / res["a_fixed_ms"], 2)
        res["host_pass_over_a_fixed"] = round(res["b_host_pass_ms"] / res["a_fixed_ms"], 2)
    if "a_fixed" in ts and "c" in ts:
        res["a_fixed_over_floor_c"] = round(res["a_fixed_ms"] / res["c_ms"], 2)
    c.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)
    if same is False:
        sys.exit(1)


if __name__ == "__main__":
    main()
