"""tools/flac_decode_rate.py on two builds of the library in alternated rounds on one box ("FLAC recordings": the
regression bound of the mono 16-bit clip decoder).  Every round is a fresh process of flac_decode_rate.py with BNHIP_LIB naming the
library, the parent's first: parent, new, parent, new, ..  A leg's figure of a round is that process's median; the new library
holds the bound when its median over the rounds is no more than the parent's median plus the spread (max - min) of the parent's own
rounds.  Both libraries must decode the burst to the source clips sample for sample (flac_decode_rate.py's own check), so their
bytes are identical.  Prints one JSON line with every round of both and writes it to --out.

    python tools/flac_decode_rate_ab.py --parent-lib PATH [--new-lib PATH] [--rounds 3] [--legs dk] [--reps 20] --out FILE
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {"d": "d_decode_pcm16_one_call", "k": "k_decode_kernels_events", "f": "f_flac_to_png_one_call", "p": "p_pcm_to_png_one_call"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--new-lib", default=os.path.join(ROOT, "birdnet-go_amd", "lib", "libbnhip.so"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--legs", default="dk")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    libs = {"parent": os.path.abspath(a.parent_lib), "new": os.path.abspath(a.new_lib)}
    runs = {"parent": [], "new": []}
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(a.rounds):
            for side in ("parent", "new"):
                out = os.path.join(tmp, f"{side}{r}.json")
                cmd = [sys.executable, os.path.join(ROOT, "tools", "flac_decode_rate.py"), "--legs", a.legs, "--reps", str(a.reps), "--out", out]
                rc = subprocess.run(cmd, env=dict(os.environ, BNHIP_LIB=libs[side]), stdout=subprocess.DEVNULL, timeout=a.timeout).returncode
                if rc != 0:                                           # (nothing more is started behind a failed round)
                    raise SystemExit(f"round {r} of the {side} library failed: exit status {rc}")
                with open(out) as fh:
                    runs[side].append(json.load(fh))
    first = runs["parent"][0]
    res = {"tool": "flac_decode_rate_ab", "rounds": a.rounds, "order": "parent, new, alternated; a fresh process each", "legs": a.legs, "reps": a.reps,
           "clips": first["clips"], "pcm_bytes": first["pcm_bytes"], "flac_bytes": first["flac_bytes"], "frames": first["frames"]}
    ok = True
    for side in ("parent", "new"):
        res[side + "_library_sha256_16"] = runs[side][0]["library_sha256_16"]
        for key in ("d_equals_clips", "k_equals_clips", "f_equals_p"):
            if key in first:
                res[f"{side}_{key}"] = all(run[key] for run in runs[side])
                ok = ok and res[f"{side}_{key}"]
    for leg in a.legs:
        name = LEGS[leg] + "_ms"
        p, n = [run[name] for run in runs["parent"]], [run[name] for run in runs["new"]]
        spread = max(p) - min(p)
        held = statistics.median(n) <= statistics.median(p) + spread
        res[LEGS[leg]] = {"parent_rounds_ms": p, "new_rounds_ms": n, "parent_median_ms": round(statistics.median(p), 3),
                          "new_median_ms": round(statistics.median(n), 3), "parent_spread_ms": round(spread, 3), "within_bound": held}
        ok = ok and held
    res["identical_decoded_bytes"] = all(res.get(f"{s}_{k}", True) for s in ("parent", "new") for k in ("d_equals_clips", "k_equals_clips"))
    line = json.dumps(res)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
