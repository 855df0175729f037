"""File analysis of a FLAC recording on the full synthetic model (DESIGN section 9 "FLAC recordings").  Main leg: an hour of 48 kHz
mono int16, encoded by the project's own device encoder at lpc_order 8 (one stream, block size 4096: about 42 000 frames) -
  (a) one bnhip_analyze_flac_topk call: the compressed bytes go up, the decoder fills the slots;
  (b) the route before this entry: bnhip_flac_decode_pcm16 (PCM back to the host), then bnhip_analyze_pcm_topk (PCM up again);
  (c) the floor: bnhip_analyze_pcm_topk on PCM the host already holds.  The decode's share of (a) is its gap to (c).
Stereo / 24-bit leg (--wide-seconds, 0 = skip): a stereo 24-bit stream written by a vectorised writer in this tool - every frame
independent channels, VERBATIM subframes (recorded in the JSON: decode time depends on the subframe kinds, and VERBATIM is the
cheapest to restore and the largest to scan) -
  (w) bnhip_analyze_flac_topk on it, (v) bnhip_analyze_channels_pcm_topk on the same PCM.
The legs run in one process, alternated round by round, host clock around calls that end in a synchronise; medians over --rounds
after one warm-up of each, every round's time kept.  (a), (b) and (c) must answer the same top-k bit for bit, and so must (w) and
(v): the tool's hard assertions.  Prints one JSON line and, with --out, writes it there.

    python tools/analyze_flac_rate.py [--minutes 60] [--wide-seconds 600] [--rounds 3] [--max-batch 256] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import birdnet_go_amd  # noqa: E402,F401
from birdnet_go_amd import flac, host, synth_model as sm, wav  # noqa: E402
from analyze_channels_rate import stereo  # noqa: E402

MODEL_RATE, CLIP, BS = 48000, 144000, 4096


def _crc_table(poly, width):
    top, mask = 1 << (width - 1), (1 << width) - 1
    t = np.zeros(256, np.uint32)
    for b in range(256):
        reg = b << (width - 8)
        for _ in range(8):
            reg = ((reg << 1) ^ poly) & mask if reg & top else (reg << 1) & mask
        t[b] = reg
    return t


def _crc_rows(rows, poly, width):
    """The CRC of every row of a uint8 matrix at once (a byte column per step)."""
    t, mask = _crc_table(poly, width), (1 << width) - 1
    reg = np.zeros(rows.shape[0], np.uint32)
    for col in range(rows.shape[1]):
        reg = ((reg << 8) & mask) ^ t[((reg >> (width - 8)) ^ rows[:, col]) & 0xFF]
    return reg


def verbatim_stereo24(frames24):
    """int32 [n, 2] samples in 24-bit range, n a multiple of BS -> a FLAC stream of independent-channel VERBATIM frames."""
    n = frames24.shape[0]
    assert n % BS == 0 and n // BS < (1 << 16)
    nf = n // BS
    num = np.arange(nf)
    head = np.zeros((nf, 8), np.uint8)                                # sync, bs code 12 / rate code 10, stereo / 24 bits, 3-byte number, CRC-8
    head[:, 0], head[:, 1], head[:, 2], head[:, 3] = 0xFF, 0xF8, 0xCA, 0x1C
    head[:, 4], head[:, 5], head[:, 6] = 0xE0 | (num >> 12), 0x80 | ((num >> 6) & 63), 0x80 | (num & 63)
    head[:, 7] = _crc_rows(head[:, :7], 0x07, 8)
    u = (frames24.astype(np.int64) & 0xFFFFFF).astype(np.uint32).reshape(nf, BS, 2)
    body = np.zeros((nf, 2, 1 + 3 * BS), np.uint8)
    body[:, :, 0] = 0x02                                              # VERBATIM, no wasted bits
    for ch in range(2):
        for k in range(3):
            body[:, ch, 1 + k::3] = (u[:, :, ch] >> (16 - 8 * k)) & 0xFF
    rows = np.concatenate([head, body.reshape(nf, -1)], axis=1)
    crc = _crc_rows(rows, 0x8005, 16)
    rows = np.concatenate([rows, (crc >> 8).astype(np.uint8)[:, None], (crc & 0xFF).astype(np.uint8)[:, None]], axis=1)
    size = rows.shape[1]
    v = (MODEL_RATE << 44) | (1 << 41) | (23 << 36) | n
    info = BS.to_bytes(2, "big") * 2 + size.to_bytes(3, "big") * 2 + v.to_bytes(8, "big") + bytes(16)
    return b"fLaC" + bytes([0x80, 0, 0, 34]) + info + rows.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=int, default=60)
    ap.add_argument("--wide-seconds", type=int, default=600)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    host.init()                                                      # no device: a loud error, not a fallback
    lib = host.load_library()
    mono = np.ascontiguousarray(stereo(a.minutes * 60)[:, 0])
    n = mono.size
    _, clip_len, hop, min_tail = wav.window_table([CLIP], MODEL_RATE, 3.0, 0.0)
    assert clip_len == CLIP
    stream = flac.encode_clips([mono], MODEL_RATE, lpc_order=flac.LEVEL5_LPC_ORDER, ragged=True)[0]
    c = host.HipClassifier(sm.build_model(sm.SynthConfig()), max_batch=a.max_batch)
    with open(host.LIB_PATH, "rb") as fh:
        digest = hashlib.sha256(fh.read()).hexdigest()[:16]
    res = {"tool": "analyze_flac_rate", "library": os.path.relpath(host.LIB_PATH, ROOT), "library_sha256_16": digest, "minutes": a.minutes,
           "rate": MODEL_RATE, "samples": int(n), "block_size": BS, "frames": -(-n // BS), "lpc_order": flac.LEVEL5_LPC_ORDER,
           "flac_bytes": len(stream), "pcm_bytes": int(mono.nbytes), "flac_over_pcm": round(len(stream) / mono.nbytes, 4), "hop": int(hop),
           "max_batch": a.max_batch, "rounds": a.rounds}
    results = {}

    def leg_a():
        conf, idx, _, _, r = c.analyze_flac_topk([stream], 0, MODEL_RATE, hop, min_tail, k=a.k)
        results["a"] = int(r[0]["status"])
        return conf, idx

    def leg_b():
        clips, r = host.flac_decode([stream])
        return c.analyze_pcm_topk(clips[0], 16, [n], hop, min_tail, k=a.k)[:2]

    def leg_c():
        return c.analyze_pcm_topk(mono, 16, [n], hop, min_tail, k=a.k)[:2]

    legs = [("a_analyze_flac", leg_a), ("b_decode_then_analyze", leg_b), ("c_pcm_floor", leg_c)]
    if a.wide_seconds:
        t0 = time.perf_counter()
        st = stereo(a.wide_seconds)
        st = st[:st.shape[0] // BS * BS]
        x24 = st.astype(np.int32) * 256 + (np.arange(st.shape[0], dtype=np.int32)[:, None] * 37 % 251)      # low bits a 16-bit word lacks
        wide = verbatim_stereo24(x24)
        u = (x24.astype(np.int64) & 0xFFFFFF).astype(np.uint32).reshape(-1)
        raw24 = np.stack([u & 255, (u >> 8) & 255, u >> 16], axis=1).astype(np.uint8).reshape(-1)
        res["wide"] = {"seconds": a.wide_seconds, "frames_of_samples": int(x24.shape[0]), "channels": 2, "bits": 24, "block_size": BS,
                       "subframes": "VERBATIM in both channels of every frame, independent channels", "flac_bytes": len(wide),
                       "pcm_bytes": int(raw24.size), "writer_s": round(time.perf_counter() - t0, 2)}
        recs = host.channel_recordings([x24.shape[0]], MODEL_RATE, 24, 2, "mix")

        def leg_w():
            conf, idx, _, _, r = c.analyze_flac_topk([wide], "mix", MODEL_RATE, hop, min_tail, k=a.k)
            results["w"] = int(r[0]["status"])
            return conf, idx

        def leg_v():
            return c.analyze_channels_pcm_topk(raw24, recs, MODEL_RATE, hop, min_tail, k=a.k)[:2]
        legs += [("w_wide_analyze_flac", leg_w), ("v_wide_channels_pcm", leg_v)]
    first = {name: f() for name, f in legs}                           # warm-up of every leg, and the comparisons
    same = lambda p, q: bool(np.array_equal(first[p][0], first[q][0]) and np.array_equal(first[p][1], first[q][1]))
    res["a_equals_b_equals_c"] = same("a_analyze_flac", "b_decode_then_analyze") and same("a_analyze_flac", "c_pcm_floor")
    ok = res["a_equals_b_equals_c"] and results["a"] == host.FLAC_OK
    if a.wide_seconds:
        res["w_equals_v"] = same("w_wide_analyze_flac", "v_wide_channels_pcm")
        ok = ok and res["w_equals_v"] and results["w"] == host.FLAC_OK
    ts = {name: [] for name, _ in legs}
    for _ in range(a.rounds):
        for name, f in legs:
            t0 = time.perf_counter()
            f()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    for name, v in ts.items():
        res[name + "_ms"] = round(float(np.median(v)), 2)
        res[name + "_rounds_ms"] = [round(t, 2) for t in v]
    res["decode_share_of_a_ms"] = round(res["a_analyze_flac_ms"] - res["c_pcm_floor_ms"], 2)
    res["a_over_b"] = round(res["a_analyze_flac_ms"] / res["b_decode_then_analyze_ms"], 3)
    if a.wide_seconds:
        res["wide_decode_share_ms"] = round(res["w_wide_analyze_flac_ms"] - res["v_wide_channels_pcm_ms"], 2)
    del lib
    c.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
