"""numpy restatement of the analysis route's processing (AudioRouter.applyProcessing, internal/audiocore/router.go:1006-1080), the
oracle of the equalizer bank tests.  Go's operation order, step by step:

  1. convert.BytesToFloat64PCM16Into: x = float64(int16) / 32768
  2. equalizer.FilterChain.ApplyBatch: for every filter, for every pass, for every sample
         y = b0*x + b1*in1 + b2*in2 - a1*out1 - a2*out2        (coefficients / a0, left to right, each op rounded)
  3. convert.ScaleFloat64Slice: y * gainLinear                  (skipped when gainLinear == 1.0: the same value)
  4. convert.Float64ToBytesPCM16: clamp to [-1, 1], int16(y * 32767) truncated toward zero
  and the route is skipped (bytes as they are) when there is no chain and the gain is 1.0 (router.go:848).

numpy's elementwise float64 ops are single IEEE operations, so vectorising across streams keeps every value Go's.  Also the RBJ
designer of equalizer.go's New* constructors in Python's math, for the designer's tolerance test.
"""
import math

import numpy as np

TYPES = ("LowPass", "HighPass", "AllPass", "BandPass", "BandReject", "LowShelf", "HighShelf", "Peaking")


def hz_to_octaves(f, width):
    half = width / 2.0
    if half >= f - 1.0:
        half = f - 1.0
    if half <= 0:
        half = 0.01
    lower = f - half
    if lower <= 0:
        lower = 0.01
    return math.log2((f + half) / lower)


def design(kind, fs, f, q=0.0, width=0.0, gain=0.0):
    """-> raw (b0, b1, b2, a0, a1, a2) of the RBJ cookbook biquad, as the reference's constructors parameterise it."""
    w0 = 2.0 * math.pi * f / fs
    c, s = math.cos(w0), math.sin(w0)
    if kind in ("BandPass", "BandReject", "Peaking"):
        alpha = s * math.sinh(math.log(2.0) / 2.0 * hz_to_octaves(f, width) * w0 / s)
    else:
        alpha = s / (2.0 * q)
    A = math.pow(10.0, gain / 40.0)
    if kind == "LowPass":
        return ((1 - c) / 2, 1 - c, (1 - c) / 2, 1 + alpha, -2 * c, 1 - alpha)
    if kind == "HighPass":
        return ((1 + c) / 2, -(1 + c), (1 + c) / 2, 1 + alpha, -2 * c, 1 - alpha)
    if kind == "AllPass":
        return (1 - alpha, -2 * c, 1 + alpha, 1 + alpha, -2 * c, 1 - alpha)
    if kind == "BandPass":
        return (alpha, 0.0, -alpha, 1 + alpha, -2 * c, 1 - alpha)
    if kind == "BandReject":
        return (1.0, -2 * c, 1.0, 1 + alpha, -2 * c, 1 - alpha)
    if kind in ("LowShelf", "HighShelf"):
        beta = math.sqrt(A) / q
        sg = 1.0 if kind == "LowShelf" else -1.0
        return (A * ((A + 1) - sg * (A - 1) * c + beta * s), sg * 2 * A * ((A - 1) - sg * (A + 1) * c),
                A * ((A + 1) - sg * (A - 1) * c - beta * s), (A + 1) + sg * (A - 1) * c + beta * s,
                -sg * 2 * ((A - 1) + sg * (A + 1) * c), (A + 1) + sg * (A - 1) * c - beta * s)
    if kind == "Peaking":
        return (1 + alpha * A, -2 * c, 1 - alpha * A, 1 + alpha / A, -2 * c, 1 - alpha / A)
    raise ValueError(kind)


def normalise(sec):
    """NewFilter's precomputed coefficients: (b0, b1, b2, a1, a2) / a0."""
    b0, b1, b2, a0, a1, a2 = (float(v) for v in sec)
    return (b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0)


class Stream:
    """One source's route: its stages (filter f, pass p, in chain order), gain and filter state."""

    def __init__(self, chain=None, gain=1.0):
        self.set_chain(chain, gain)

    def set_chain(self, chain, gain=1.0):
        self.chain = list(chain or [])
        self.stages = [normalise(sec) for sec, passes in self.chain for _ in range(passes)]
        self.gain = float(gain)
        self.reset()

    def reset(self):
        self.state = np.zeros((len(self.stages), 4))     # in1, in2, out1, out2 per stage

    @property
    def passthrough(self):
        return not self.stages and self.gain == 1.0


def process(streams, frames):
    """streams: {id: Stream}; frames: [(id, int16 array | bytes), ...] in call order -> [int16 array, ...] per frame.  State
    carries over in the Stream objects, as the bank's does."""
    arrs = [np.frombuffer(f, "<i2") if isinstance(f, (bytes, bytearray)) else np.asarray(f, np.int16).reshape(-1) for _, f in frames]
    ids = []
    for sid, _ in frames:
        if sid not in ids:
            ids.append(sid)
    work = [i for i in ids if not streams[i].passthrough]
    cat = {i: np.concatenate([a for (s, _), a in zip(frames, arrs) if s == i] + [np.zeros(0, np.int16)]) for i in ids}
    out = {i: cat[i] for i in ids}
    if work:
        N, T = len(work), max(cat[i].size for i in work)
        S = max(len(streams[i].stages) for i in work)
        lens = np.array([cat[i].size for i in work])
        X = np.zeros((N, T))
        for k, i in enumerate(work):
            X[k, :cat[i].size] = cat[i].astype(np.float64) / 32768.0
        for s in range(S):
            has = np.array([s < len(streams[i].stages) for i in work])
            co = np.array([streams[i].stages[s] if s < len(streams[i].stages) else (1.0, 0.0, 0.0, 0.0, 0.0) for i in work]).T
            st = np.array([streams[i].state[s] if s < len(streams[i].stages) else np.zeros(4) for i in work]).T.copy()
            b0, b1, b2, a1, a2 = co
            in1, in2, out1, out2 = st
            for t in range(T):
                x = X[:, t]
                y = b0 * x + b1 * in1 + b2 * in2 - a1 * out1 - a2 * out2
                act = has & (t < lens)
                in2 = np.where(act, in1, in2)
                in1 = np.where(act, x, in1)
                out2 = np.where(act, out1, out2)
                out1 = np.where(act, y, out1)
                X[:, t] = np.where(act, y, x)
            for k, i in enumerate(work):
                if s < len(streams[i].stages):
                    streams[i].state[s] = (in1[k], in2[k], out1[k], out2[k])
        for k, i in enumerate(work):
            y = X[k, :lens[k]]
            g = streams[i].gain
            if g != 1.0:
                y = y * g
            y = np.minimum(np.maximum(y, -1.0), 1.0)
            out[i] = np.trunc(y * 32767.0).astype(np.int16)
    res, taken = [], {i: 0 for i in ids}
    for (sid, _), a in zip(frames, arrs):
        res.append(out[sid][taken[sid]:taken[sid] + a.size])
        taken[sid] += a.size
    return res
