"""The clip loudness spec of DESIGN.md §9 restated: numpy / Python float64, the serial recurrence, explicit loops wherever the
order of operations matters.  Every multiply and add below is its own rounded operation (CPython and numpy never fuse).

  measure(s, rate)                  the spec in float64: sub-block energies, block energies, both gates, loudness, true peak
  measure(s, rate, go32=True)       the Go meter (audionorm/meter.go, truepeak.go) line by line in float32; its two SIMD sums
                                    (f32.SumOfSquares, ConvolveValidMaxAbsMulti), whose order is not in the tree, run sequentially
  normalize(s, rate, ...)           measure, PlanGain, gate fallback with the lifted clip measured again, clamp, pcmgain
"""
import math

import numpy as np

INF = math.inf
PEAK_LIMITED, GATE_LIFTED, CLAMPED = 1, 2, 4
F32 = np.float32


def sub_block(rate):
    """Go's math.Round(0.1 * rate): 11 025 Hz -> 1103 (Python's round gives 1102)."""
    return int(math.floor(0.1 * float(rate) + 0.5))


def kweight64(rate):
    """kWeightingStages in double (kweight.go:32-68): (b0 b1 b2 a1 a2) of the shelf, then of the high-pass."""
    fs = float(rate)
    f0, q, gdb, vbex = 1681.974450955533, 0.7071752369554196, 3.999843853973347, 0.4996667741545416
    K = math.tan(math.pi * f0 / fs)
    Vh = math.pow(10.0, gdb / 20.0)
    Vb = math.pow(Vh, vbex)
    K2 = K * K
    a0 = 1.0 + K / q + K2
    s1 = [(Vh + Vb * K / q + K2) / a0, 2.0 * (K2 - Vh) / a0, (Vh - Vb * K / q + K2) / a0, 2.0 * (K2 - 1.0) / a0, (1.0 - K / q + K2) / a0]
    f0, q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    K2 = K * K
    a0 = 1.0 + K / q + K2
    s2 = [1.0, -2.0, 1.0, 2.0 * (K2 - 1.0) / a0, (1.0 - K / q + K2) / a0]
    return s1 + s2


def kweight(rate):
    """The coefficients the meter runs with: float32 (meter.go:45-50), here widened to Python floats."""
    return [float(F32(c)) for c in kweight64(rate)]


def _bessel_i0(x):
    s, term, half = 1.0, 1.0, x / 2.0
    for k in range(1, 40):
        term *= (half / k) * (half / k)
        s += term
        if term < 1e-15 * s:
            break
    return s


def tp_coef64():
    """buildTruePeakKernel (truepeak.go:55-110): [4][32], Kaiser beta 9, each phase divided by its sum."""
    P, T = 4, 32
    L = P * T
    center = (L - 1) / 2.0
    proto = []
    for n in range(L):
        x = (n - center) / P
        sinc = 1.0 if x == 0 else math.sin(math.pi * x) / (math.pi * x)
        r = 2.0 * n / (L - 1) - 1.0
        proto.append(sinc * (_bessel_i0(9.0 * math.sqrt(1.0 - r * r)) / _bessel_i0(9.0)))
    k = np.zeros((P, T))
    for p in range(P):
        s = 0.0
        for t in range(T):
            s += proto[p + P * t]
        for t in range(T):
            k[p, t] = proto[p + P * t] / s if s != 0 else proto[p + P * t]
    return k


def tp_coef():
    """tpKernelRev's values (float32), widened."""
    return tp_coef64().astype(F32).astype(np.float64)


GATE_ABS = float(F32(math.pow(10.0, (-70.0 - -0.691) / 10.0)))      # absGateEnergy (meter.go:27-34)
GATE_REL = float(F32(math.pow(10.0, -10.0 / 10.0)))                  # relGateEnergyFactor


def round_half_away(v):
    """math.Round on an array: exact, half away from zero (v - trunc(v) is exact)."""
    t = np.trunc(v)
    return t + np.where(np.abs(v - t) >= 0.5, np.sign(v), 0.0)


def apply_gain(s, factor):
    """pcmgain.ApplyInt16 (pcmgain.go:52-63): (double)s * factor, rounded half away, saturated; factor 1 is a copy."""
    s = np.asarray(s, np.int16)
    if factor == 1.0:
        return s.copy()
    return np.clip(round_half_away(s.astype(np.float64) * float(factor)), -32768.0, 32767.0).astype(np.int16)


def factor_from_db(gain_db):
    return 1.0 if gain_db == 0 else math.pow(10.0, gain_db / 20.0)


def sub_energies(s, rate, go32=False):
    """E[k] of the K-weighted clip: the serial recurrence from zero state, y^2 summed in sample order per sub-block."""
    S = sub_block(rate)
    Ns = len(s) // S
    if go32:
        c = [F32(v) for v in kweight64(rate)]
        xs = [F32(v) * F32(1.0 / 32768.0) for v in np.asarray(s[:Ns * S], np.int16)]
        zero = F32(0.0)
    else:
        c = kweight(rate)
        xs = (np.asarray(s[:Ns * S], np.int16).astype(np.float64) / 32768.0).tolist()
        zero = 0.0
    b0, b1, b2, a1, a2, d0, d1, d2, e1, e2 = c
    x1 = x2 = u1 = u2 = y1 = y2 = zero
    E = []
    for k in range(Ns):
        acc = zero
        for x in xs[k * S:(k + 1) * S]:
            u = b0 * x + b1 * x1 + b2 * x2 - a1 * u1 - a2 * u2
            y = d0 * u + d1 * u1 + d2 * u2 - e1 * y1 - e2 * y2
            x2, x1 = x1, x
            u2, u1 = u1, u
            y2, y1 = y1, y
            acc = acc + y * y
        E.append(acc)
    return np.array(E, F32 if go32 else np.float64)


def block_energies(E, S, go32=False):
    """z[j] = (E[j] + E[j+1] + E[j+2] + E[j+3]) / (4 S), left to right."""
    Nb = len(E) - 3
    if Nb <= 0:
        return np.zeros(0, F32 if go32 else np.float64)
    den = F32(4 * S) if go32 else float(4 * S)
    return (((E[0:Nb] + E[1:Nb + 1]) + E[2:Nb + 2]) + E[3:Nb + 3]) / den


def gated_loudness(z, go32=False):
    """Both gates in block order (meter.go:318-352) -> (L, relative gate or None)."""
    A, R = (F32(GATE_ABS), F32(GATE_REL)) if go32 else (GATE_ABS, GATE_REL)
    zero = F32(0.0) if go32 else 0.0
    s, cnt = zero, 0
    for zj in z:
        if zj > A:
            s = s + zj
            cnt += 1
    if cnt == 0:
        return -INF, None
    g = (s / (F32(cnt) if go32 else float(cnt))) * R
    s2, cnt2 = zero, 0
    for zj in z:
        if zj > A and zj > g:
            s2 = s2 + zj
            cnt2 += 1
    if cnt2 == 0:
        return -INF, float(g)
    return -0.691 + 10.0 * math.log10(float(s2) / float(cnt2)), float(g)


def gate_margin(z, g):
    """Smallest relative distance of any block energy from the absolute gate and (when there is one) from the relative gate."""
    z = np.asarray(z, np.float64)
    if z.size == 0:
        return INF
    m = float(np.min(np.abs(z - GATE_ABS) / GATE_ABS))
    if g is not None:
        m = min(m, float(np.min(np.abs(z - g) / g)))
    return m


def true_peak(s, go32=False):
    """max(|x|, |sum_t c[p][t] x[k - t]|) over p = 0..3, k = 0..n + 15; each sum from 0.0, oldest sample first (t = 31 .. 0)."""
    dt = F32 if go32 else np.float64
    x = np.asarray(s, np.int16).astype(dt) * dt(1.0 / 32768.0)
    n = len(x)
    c = tp_coef64().astype(F32).astype(dt)
    xp = np.concatenate([np.zeros(31, dt), x, np.zeros(16, dt)])
    P = dt(np.max(np.abs(x))) if n else dt(0)
    for p in range(4):
        acc = np.zeros(n + 16, dt)
        for t in range(31, -1, -1):
            acc = acc + c[p, t] * xp[31 - t:31 - t + n + 16]
        P = max(P, dt(np.max(np.abs(acc))))
    return float(P)


def measure(s, rate, go32=False):
    S = sub_block(rate)
    E = sub_energies(s, rate, go32)
    z = block_energies(E, S, go32)
    L, g = gated_loudness(z, go32)
    P = true_peak(s, go32)
    return {"L": L, "P": P, "dbtp": 20.0 * math.log10(P) if P > 0 else -INF, "E": E.astype(np.float64), "z": z.astype(np.float64),
            "rel_gate": g, "margin": gate_margin(z, g)}


def plan_gain(L, dbtp, T, C):
    """PlanGain (audionorm.go:181-202) -> (target_gain, gain, limited)."""
    if L == -INF:
        return 0.0, 0.0, False
    tg = T - L
    gain, limited = tg, False
    if dbtp != -INF:
        head = C - dbtp
        if gain > head:
            gain, limited = head, True
    return tg, gain, limited


def normalize(s, rate, T=-23.0, C=-1.0, max_gain=30.0, gate_fallback=False, lift_db=None, m=None):
    """The whole plan.  lift_db: build the lifted clip from this (reported) lift instead of the restatement's own; m: a measurement
    of s made before.  -> dict with the fields of bnhip_loudness, "margin" (the smallest gate distance of any measurement made)
    and "lifted" (the second measurement, or None)."""
    m = m or measure(s, rate)
    r = {"integrated_lufs": m["L"], "true_peak_dbtp": m["dbtp"], "true_peak": m["P"], "margin": m["margin"], "lifted": None}
    flags, lift, Lm = 0, 0.0, m["L"]
    if gate_fallback and m["L"] == -INF and m["P"] > 0:
        own = min(C - m["dbtp"], T + 70.0)
        r["own_lift_db"] = own
        lift = own if lift_db is None else lift_db
        flags |= GATE_LIFTED
        m2 = measure(apply_gain(s, factor_from_db(lift)), rate)
        r["lifted"], r["margin"], Lm = m2, min(m["margin"], m2["margin"]), m2["L"]
        tg, gain, limited = plan_gain(m2["L"], m2["dbtp"], T, C)
        planned = lift + gain if m2["L"] != -INF else lift
    else:
        tg, planned, limited = plan_gain(m["L"], m["dbtp"], T, C)
    if limited:
        flags |= PEAK_LIMITED
    lim = abs(max_gain)
    gain_db = planned
    if planned > lim:
        gain_db, flags = lim, flags | CLAMPED
    elif planned < -lim:
        gain_db, flags = -lim, flags | CLAMPED
    r.update(target_gain_db=tg, lift_db=lift, planned_gain_db=planned, gain_db=gain_db, factor=factor_from_db(gain_db),
             output_lufs=-INF if Lm == -INF else Lm + (gain_db - lift), flags=flags)
    return r


def sine_int16(dbfs, hz, seconds, rate, phase=0.0):
    """A sine of peak 10^(dbfs / 20), rounded to int16 (the reference tests' sineInt16)."""
    n = int(round(seconds * rate))
    a = math.pow(10.0, dbfs / 20.0)
    v = a * np.sin(2.0 * np.pi * hz * np.arange(n) / rate + phase) * 32767.0
    return np.clip(np.round(v), -32768, 32767).astype(np.int16)
