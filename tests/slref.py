"""Restatement of the 1/3-octave sound level monitor (soundlevel.Processor, internal/audiocore/soundlevel/processor.go) in Go's
operation order, the oracle of the sound level bank tests:

  1. bands (NewProcessor :120-158, newOctaveBandFilter :161-225): the ISO 266 centres whose upper edge c * 2^(1/6) lies below
     0.95 x Nyquist; RBJ constant-0-dB band-pass, Q = max(c / (high - low), 0.5), every coefficient / a0
  2. per sample (processAudioSample :231-250): x = float64(int16) / 32768;
         y = b0*x + b1*x1 + b2*x2 - a1*y1 - a2*y2     (left to right, each op rounded, the b1 term kept)
     NaN, +-Inf or |y| > 100: state zeroed, y = x * 0.1; then x2 = x1, x1 = x, y2 = y1, y1 = y
  3. per call (ProcessSamples :258-327): the outputs are appended to the second buffer; if it holds fs samples, ONE measurement
     of its first fs: sum += s*s from 0.0, rms = sqrt(sum / fs), clamped to [1e-10, 10], dB = 20 * (log(rms) * (1/Ln10))
  4. every `interval` measurements one report: per band min, max, mean (sum / len) in slot order (:349-412)

The filter outputs and block sums do not depend on frame boundaries, only the emission schedule does: each stream's frames are
filtered back to back (numpy across streams x bands, one time step at a time: numpy's elementwise float64 ops are single IEEE
operations; or tests/native/soundlevel_ref.c for long cases), then the frames are replayed in Python.
"""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np

INV_LN10 = float.fromhex("0x1.bcb7b1526e50ep-2")        # Go's 1/Ln10 (math.Log10 = math.Log(x) * (1/Ln10))
CENTRES = (25, 31.5, 40, 50, 63, 80, 100, 125, 160, 200, 250, 315, 400, 500, 630, 800,
           1000, 1250, 1600, 2000, 2500, 3150, 4000, 5000, 6300, 8000, 10000, 12500, 16000, 20000)
NATIVE_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "soundlevel_ref.c")


def design(rate):
    """-> [(c, b0, b1, b2, a1, a2), ...] as NewProcessor builds its filters, with Python's math (the C library's)."""
    fs = float(rate)
    nyquist = fs / 2.0
    threshold = nyquist * 0.95
    out = []
    for c in CENTRES:
        c = float(c)
        if c * math.pow(2.0, 1.0 / 6.0) >= threshold:
            continue
        low, high = c / math.pow(2.0, 1.0 / 6.0), c * math.pow(2.0, 1.0 / 6.0)
        if low <= 0 or high >= nyquist:
            raise ValueError(f"band {c} out of range")
        omega = 2.0 * math.pi * c / fs
        so, co = math.sin(omega), math.cos(omega)
        q = c / (high - low)
        if q < 0.5:
            q = 0.5
        alpha = so / (2.0 * q)
        a0 = 1.0 + alpha
        r = (c, alpha / a0, 0.0 / a0, -alpha / a0, -2.0 * co / a0, (1.0 - alpha) / a0)
        if abs(r[5]) >= 1.0 or abs(r[4]) >= 1.0 + r[5]:
            raise ValueError(f"band {c} unstable")
        out.append(r)
    return out


def band_key(hz):
    """formatBandKey (:440-445)."""
    return "%.1f_Hz" % hz if hz < 1000 else "%.1f_kHz" % (hz / 1000)


def db(s, fs):
    rms = math.sqrt(s / fs)
    if rms < 1e-10:
        rms = 1e-10
    elif rms > 10.0:
        rms = 10.0
    v = 20 * (math.log(rms) * INV_LN10)
    return v if math.isfinite(v) else -100.0


class Processor:
    """One source's Processor: filter state, the open block's fill, the unmeasured count, finished blocks, interval slots."""

    def __init__(self, rate, interval=10, table=None):
        self.fs = int(rate)
        self.table = [tuple(float(v) for v in b) for b in (table if table is not None else design(rate))]
        self.interval = max(int(interval), 1)
        self.reset()

    def reset(self):
        nb = len(self.table)
        self.st = np.zeros((nb, 5))              # x1, x2, y1, y2, sum of the open block
        self.fill = 0
        self.unmeasured = 0
        self.fifo = []
        self.count = 0
        self.slots = []

    @property
    def coef(self):
        return np.array([b[1:] for b in self.table], np.float64)


def _filter_numpy(procs, xs):
    """procs: [Processor] of one rate, xs: [int16 array] -> [[block sums array, ...] per stream]; state advances."""
    fs, nb = procs[0].fs, len(procs[0].table)
    N, T = len(procs), max([x.size for x in xs] + [0])
    lens = np.array([x.size for x in xs])
    X = np.zeros((N, max(T, 1)))
    for k, x in enumerate(xs):
        X[k, :x.size] = x.astype(np.float64) / 32768.0
    co = np.stack([p.coef for p in procs])                       # (N, nb, 5)
    b0, b1, b2, a1, a2 = (co[:, :, i] for i in range(5))
    st = np.stack([p.st for p in procs])
    x1, x2, y1, y2, s = (st[:, :, i].copy() for i in range(5))
    fill = np.array([p.fill for p in procs])
    out = [[] for _ in procs]
    for t in range(T):
        act1 = t < lens
        act = act1[:, None]
        x = X[:, t:t + 1]
        y = b0 * x + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        bad = ~(np.abs(y) <= 100.0) & act
        if bad.any():
            x1, x2, y1, y2 = (np.where(bad, 0.0, v) for v in (x1, x2, y1, y2))
            y = np.where(bad, x * 0.1, y)
        x2 = np.where(act, x1, x2)
        x1 = np.where(act, x, x1)
        y2 = np.where(act, y1, y2)
        y1 = np.where(act, y, y1)
        s = np.where(act, s + y * y, s)
        fill = fill + act1
        done = np.nonzero(fill == fs)[0]
        for k in done:
            out[k].append(s[k].copy())
            s[k] = 0.0
            fill[k] = 0
    for k, p in enumerate(procs):
        p.st = np.stack([x1[k], x2[k], y1[k], y2[k], s[k]], 1)
        p.fill = int(fill[k])
    return out


_native = None


def _native_lib():
    global _native
    if _native is None:
        d = tempfile.mkdtemp(prefix="slref")
        so = os.path.join(d, "libslref.so")
        subprocess.check_call(["cc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", NATIVE_SRC, "-o", so, "-lm"])
        lib = C.CDLL(so)
        lib.sl_filter.restype = C.c_long
        lib.sl_filter.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.POINTER(C.c_long), C.c_void_p, C.c_long]
        _native = lib
    return _native


def _filter_native(procs, xs):
    lib = _native_lib()
    out = []
    for p, x in zip(procs, xs):
        x = np.ascontiguousarray(x, np.int16)
        nb = len(p.table)
        coef = np.ascontiguousarray(p.coef)
        st = np.ascontiguousarray(p.st)
        cap = (p.fill + x.size) // p.fs + 1
        sums = np.zeros((cap, nb))
        fill = C.c_long(p.fill)
        k = lib.sl_filter(coef.ctypes.data, nb, p.fs, x.ctypes.data if x.size else None, x.size, st.ctypes.data, C.byref(fill),
                          sums.ctypes.data, cap)
        p.st, p.fill = st, int(fill.value)
        out.append([sums[i].copy() for i in range(k)])
    return out


def _report(p, stream, frame):
    bands = {}
    n = p.count
    for j, b in enumerate(p.table):
        vals = [p.slots[k][j] for k in range(n)]
        lo = hi = vals[0]
        tot = 0.0
        for v in vals:
            if not math.isfinite(v):
                continue
            if v < lo:
                lo = v
            if v > hi:
                hi = v
            tot += v
        mean = tot / n
        fix = lambda v: v if math.isfinite(v) else -100.0
        bands[band_key(b[0])] = {"center_frequency_hz": b[0], "min_db": fix(lo), "max_db": fix(hi), "mean_db": fix(mean),
                                 "sample_count": n}
    return {"stream": stream, "frame": frame, "duration_seconds": p.interval, "octave_bands": bands}


def process(procs, frames, native=None):
    """procs: {id: Processor}; frames: [(id, int16 array | bytes), ...] in call order -> reports in frame order, each as
    host.SoundLevelBank.process gives them.  State carries over in the Processor objects.  native: filter with the C restatement
    (default: when the call has more than 48 000 samples of one stream)."""
    arrs = [np.frombuffer(f, "<i2") if isinstance(f, (bytes, bytearray)) else np.asarray(f, np.int16).reshape(-1) for _, f in frames]
    ids = []
    for sid, _ in frames:
        if sid not in ids:
            ids.append(sid)
    cat = {i: np.concatenate([a for (s, _), a in zip(frames, arrs) if s == i] + [np.zeros(0, np.int16)]) for i in ids}
    if native is None:
        native = any(c.size > 48000 for c in cat.values())
    fills = {i: procs[i].fill for i in ids}
    blocks = {}
    by_rate = {}
    for i in ids:
        by_rate.setdefault(procs[i].fs, []).append(i)
    for _, group in by_rate.items():
        res = (_filter_native if native else _filter_numpy)([procs[i] for i in group], [cat[i] for i in group])
        for i, r in zip(group, res):
            blocks[i] = r
    taken = {i: 0 for i in ids}
    reports = []
    for f, ((sid, _), a) in enumerate(zip(frames, arrs)):
        p = procs[sid]
        k = (fills[sid] + a.size) // p.fs                         # blocks this frame completes
        fills[sid] = (fills[sid] + a.size) % p.fs
        p.fifo.extend(blocks[sid][taken[sid]:taken[sid] + k])
        taken[sid] += k
        if a.size == 0:
            continue
        p.unmeasured += a.size
        if p.unmeasured < p.fs:
            continue
        p.unmeasured -= p.fs
        sums = p.fifo.pop(0)
        p.slots.append([db(float(v), p.fs) for v in sums])
        p.count += 1
        if p.count >= p.interval:
            reports.append(_report(p, sid, f))
            p.count = 0
            p.slots = []
    return reports
