"""The audio level bank at the size of a 256-source station ("Audio level"): --sources sources x 1.5 s of 48 kHz
int16 per tick, host clock around calls that end in their synchronise, p50 / p95 over --calls ticks after two warm-ups, in --rounds
rounds.  One mode per process:

  --mode process  (a) bnhip_level_bank_process_pcm alone.
  --mode fused    (b) bnhip_capture_bank_write_levels against bnhip_capture_bank_write of the same frames, alternated call by call.
                  The two forms' records and ring bytes are compared once (asserted).
  --mode parent   (c) bnhip_capture_bank_write of this build against the same entry of --parent-lib (the parent commit's library),
                  alternated call by call; "spread" is the parent's own p50 spread between the rounds.
  --mode host     (d) tools/level_ref.c, built with cc -O2: the same measurement as a plain one-thread C loop.
  --mode levels   --calls process calls and nothing else: the process for a kernel trace, whose k_frame_levels rows are the kernel's time.
Prints one JSON line; --all runs the modes (a)-(d) as child processes and writes them into --out.

    python tools/level_rate.py --mode process|fused|parent|host|levels [--sources 256] [--calls 40] [--rounds 3] [--parent-lib PATH]
    python tools/level_rate.py --all --parent-lib PATH --out profiles/rNN_level_rate.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import birdnet_go_amd  # noqa: E402,F401
from birdnet_go_amd import host  # noqa: E402

RATE = 48000


def stats(ts):
    ts = np.asarray(ts)
    return {"p50_ms": round(float(np.percentile(ts, 50)), 3), "p95_ms": round(float(np.percentile(ts, 95)), 3), "min_ms": round(float(ts.min()), 3),
            "max_ms": round(float(ts.max()), 3), "n": int(ts.size)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def tick_frames(rng, n_src, n):
    base = (np.clip(rng.normal(0, 0.1, n + n_src), -1, 1) * 32767).astype("<i2")
    return [(s, base[s:s + n].tobytes()) for s in range(n_src)]


def rounds_of(legs, calls, rounds):
    """legs: {name: fn}, run alternated call by call -> {name: [stats per round]}"""
    out = {k: [] for k in legs}
    for fn in legs.values():
        fn(), fn()                                                        # warm-up
    for _ in range(rounds):
        ts = {k: [] for k in legs}
        for _ in range(calls):
            for k, fn in legs.items():
                ts[k].append(timed(fn))
        for k in legs:
            out[k].append(stats(ts[k]))
    return out


def raw_write(lib, n_src, seconds, frames):
    """bnhip_capture_bank_write of `lib` (any build) on a bank of its own -> the call as a function"""
    vp, ci, i64 = C.c_void_p, C.c_int, C.c_int64
    lib.bnhip_init.argtypes = [C.POINTER(ci)]
    lib.bnhip_capture_bank_create.argtypes = [ci, ci, i64, ci, C.POINTER(vp)]
    lib.bnhip_capture_bank_write.argtypes = [vp, ci, vp, vp, vp, ci]
    n_dev = ci(0)
    assert lib.bnhip_init(C.byref(n_dev)) == 0 and n_dev.value >= 1
    h = vp()
    assert lib.bnhip_capture_bank_create(0, n_src, int(seconds * RATE), RATE, C.byref(h)) == 0
    keep, n, ptr = host._pcm_frames([f for _, f in frames], 16, whole=True)
    src = np.array([s for s, _ in frames], np.int32)

    def call():
        assert lib.bnhip_capture_bank_write(h, len(keep), src.ctypes.data, n.ctypes.data, ptr, 16) == 0
    call.keep = (keep, n, ptr, src, h)
    return call


def run_all(a):
    res = {"what": __doc__.split("\n\n")[0], "sources": a.sources, "calls": a.calls, "rounds": a.rounds}
    for mode in ("process", "fused", "parent", "host"):
        cmd = [sys.executable, os.path.abspath(__file__), "--mode", mode, "--sources", str(a.sources), "--calls", str(a.calls), "--rounds", str(a.rounds)]
        if a.parent_lib:
            cmd += ["--parent-lib", a.parent_lib]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(p.returncode)
        res[mode] = json.loads(p.stdout.strip().splitlines()[-1])
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["process", "fused", "parent", "host", "levels"])
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--sources", type=int, default=256)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.all:
        return run_all(a)
    tick = int(1.5 * RATE)
    out = {"mode": a.mode, "sources": a.sources, "bytes_per_call": a.sources * tick * 2}
    if a.mode == "host":
        with tempfile.TemporaryDirectory() as d:
            exe = os.path.join(d, "level_ref")
            subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-o", exe, os.path.join(ROOT, "tools", "level_ref.c"), "-lm"])
            out.update(json.loads(subprocess.check_output([exe, str(a.sources), str(tick), str(a.calls)], text=True)),
                       note="plain C loop, one thread, -O2: stands in for the Go loop, nothing more")
        print(json.dumps(out))
        return
    host.init()                                                          # no device: a loud error, not a fallback
    rng = np.random.default_rng(1)
    frames = tick_frames(rng, a.sources, tick)
    if a.mode in ("process", "levels"):
        bank = host.LevelBank(a.sources)
        items = [(bank.add_stream(), f) for _, f in frames]
        if a.mode == "levels":
            out.update(call=stats([timed(lambda: bank.process(items)) for _ in range(a.calls + 2)][2:]))
        else:
            out.update(rounds=rounds_of({"process": lambda: bank.process(items)}, a.calls, a.rounds)["process"])
        bank.close()
    elif a.mode == "fused":
        cap, twin, bank = host.CaptureBank(a.sources, 16.0, RATE), host.CaptureBank(a.sources, 16.0, RATE), host.LevelBank(a.sources)
        streams = [bank.add_stream() for _ in frames]
        recs = cap.write(frames, levels=(bank, streams))
        twin.write(frames)
        alone = host.LevelBank(a.sources)
        want = alone.process([(alone.add_stream(), f) for _, f in frames])
        assert recs.tobytes() == want.tobytes()
        spans = np.zeros(a.sources, host.CLIP_SPAN)
        for s in range(a.sources):
            spans[s] = (0, tick, s)
        assert all(np.array_equal(x, y) for x, y in zip(cap.read(spans), twin.read(spans)))
        r = rounds_of({"write_levels": lambda: cap.write(frames, levels=(bank, streams)), "write": lambda: twin.write(frames)}, a.calls, a.rounds)
        out.update(r, records_and_rings_equal=True)
    else:
        if not a.parent_lib or not os.path.exists(a.parent_lib):
            sys.exit("--mode parent needs --parent-lib, the parent commit's libbnhip.so")
        legs = {"parent": raw_write(C.CDLL(os.path.abspath(a.parent_lib)), a.sources, 16.0, frames),
                "new": raw_write(host.load_library(), a.sources, 16.0, frames)}
        r = rounds_of(legs, a.calls, a.rounds)
        p50 = [x["p50_ms"] for x in r["parent"]]
        out.update(r, parent_p50_spread_ms=round(max(p50) - min(p50), 3))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
