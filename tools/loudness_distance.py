"""The three measured distances of the clip loudness path, over tone / noise with a quiet third / modulated noise
at amplitudes 0.001 .. 0.9 and rates 8 / 24 / 48 / 256 kHz:
  scan_vs_serial      the time-parallel form (zero-state segments, 4 x 4 state scan, second pass) restated in Python float64 against
                      the serial recurrence of tests/loudref.py: integrated loudness (LU) and per-sub-block energy (relative to the
                      clip's largest);
  device_vs_spec      bnhip_loudness_measure_pcm16 against tests/loudref.py (needs the device; skipped with --no-device);
  spec_vs_go32        tests/loudref.py's float64 spec against its float32 restatement of the Go meter.
Prints one JSON line and writes it to --out.

    python tools/loudness_distance.py [--seconds 3] [--no-device] [--out profiles/r13_loudness_distance.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import loudref as R  # noqa: E402


def run(c, xs, x1, x2, u1, u2, y1, y2):
    """The cascade over xs from the given state -> (end state (u1, u2, y1, y2), sum of y^2)."""
    b0, b1, b2, a1, a2, d0, d1, d2, e1, e2 = c
    acc = 0.0
    for x in xs:
        u = b0 * x + b1 * x1 + b2 * x2 - a1 * u1 - a2 * u2
        y = d0 * u + d1 * u1 + d2 * u2 - e1 * y1 - e2 * y2
        x2, x1 = x1, x
        u2, u1 = u1, u
        y2, y1 = y1, y
        acc = acc + y * y
    return (u1, u2, y1, y2), acc


def split(n_clips, n, S):
    """loudness_split of csrc/loudness.hip: segments per sub-block."""
    for q in (8, 4, 2):
        if S % q == 0 and n_clips * (n // S) * q <= 1 << 18:
            return q
    return 1


def scanned_energies(s, rate):
    """csrc/loudness.hip's mapping, operation for operation: q segments per sub-block, zero-state pass, scan, second pass, the
    segment sums of a sub-block added in order."""
    S = R.sub_block(rate)
    Ns = len(s) // S
    q = split(1, len(s), S)
    Sq, Nq = S // q, Ns * q
    c = R.kweight(rate)
    x = (np.asarray(s, np.int16).astype(np.float64) / 32768.0).tolist()
    M = [[0.0] * 4 for _ in range(4)]
    for j in range(4):
        st = [0.0] * 4
        st[j] = 1.0
        end, _ = run(c, [0.0] * Sq, 0.0, 0.0, *st)
        for i in range(4):
            M[i][j] = end[i]
    hist = lambda k: (x[k * Sq - 1], x[k * Sq - 2]) if k else (0.0, 0.0)
    zs = [run(c, x[k * Sq:(k + 1) * Sq], *hist(k), 0.0, 0.0, 0.0, 0.0)[0] for k in range(Nq)]
    v, Ep = [0.0] * 4, []
    for k in range(Nq):
        Ep.append(run(c, x[k * Sq:(k + 1) * Sq], *hist(k), *v)[1])
        v = [zs[k][i] + (M[i][0] * v[0] + M[i][1] * v[1] + M[i][2] * v[2] + M[i][3] * v[3]) for i in range(4)]
    E = []
    for k in range(Ns):
        a = Ep[k * q]
        for i in range(1, q):
            a = a + Ep[k * q + i]
        E.append(a)
    return np.array(E)


def signals(rate, seconds, seed):
    rng = np.random.default_rng(seed)
    n = int(seconds * rate)
    t = np.arange(n) / rate
    out = []
    for amp in (0.001, 0.03, 0.9):
        out.append(("tone", amp, amp * np.sin(2 * np.pi * 997.0 * t)))
        x = amp / 3.0 * rng.standard_normal(n)
        x[n // 3:2 * n // 3] *= 1e-3
        out.append(("noise_quiet_third", amp, x))
        out.append(("modulated_noise", amp, amp / 3.0 * rng.standard_normal(n) * (0.55 + 0.45 * np.sin(2 * np.pi * 1.3 * t))))
    return [(k, a, np.round(np.clip(x, -1.0, 1.0) * 32767.0).astype(np.int16)) for k, a, x in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_loudness_distance.json"))
    a = ap.parse_args()
    if not a.no_device:
        import birdnet_go_amd  # noqa: F401
        from birdnet_go_amd import host
        host.init()
    d = {"scan_vs_serial": {"lufs": 0.0, "sub_energy_rel": 0.0}, "spec_vs_go32": {"lufs": 0.0, "dbtp": 0.0},
         "device_vs_spec": {"lufs": 0.0, "dbtp": 0.0, "sub_energy_rel": 0.0, "true_peak_bit_equal": True}}
    up = lambda k, f, v: d[k].__setitem__(f, max(d[k][f], float(v)))
    cases = 0
    for rate in (8000, 24000, 48000, 256000):
        seconds = min(a.seconds, 1.2) if rate == 256000 else a.seconds
        for kind, amp, s in signals(rate, seconds, rate):
            cases += 1
            m = R.measure(s, rate)
            S = R.sub_block(rate)
            Es = scanned_energies(s, rate)
            Ls, _ = R.gated_loudness(R.block_energies(Es, S))
            if m["L"] != -math.inf:
                up("scan_vs_serial", "lufs", abs(Ls - m["L"]))
            up("scan_vs_serial", "sub_energy_rel", np.abs(Es - m["E"]).max() / m["E"].max())
            if rate <= 48000:                                            # (the float32 scalar loop is the slow one)
                g = R.measure(s, rate, go32=True)
                if m["L"] != -math.inf:
                    up("spec_vs_go32", "lufs", abs(g["L"] - m["L"]))
                up("spec_vs_go32", "dbtp", abs(g["dbtp"] - m["dbtp"]))
            if not a.no_device:
                (r,), sub = host.loudness_measure(s, rate, sub_energy=True)
                if m["L"] != -math.inf:
                    up("device_vs_spec", "lufs", abs(r.integrated_lufs - m["L"]))
                up("device_vs_spec", "dbtp", abs(r.true_peak_dbtp - m["dbtp"]))
                up("device_vs_spec", "sub_energy_rel", np.abs(sub[0] - m["E"]).max() / m["E"].max())
                d["device_vs_spec"]["true_peak_bit_equal"] &= r.true_peak == m["P"]
    if a.no_device:
        d["device_vs_spec"] = "not measured (--no-device)"
    res = {"tool": "loudness_distance", "seconds": a.seconds, "seconds_at_256k": min(a.seconds, 1.2), "cases": cases,
           "rates": [8000, 24000, 48000, 256000], "amplitudes": [0.001, 0.03, 0.9], **d}
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
