"""The restatement of the multichannel sample rule (include/bnhip.h, bnhip_analyze_channels_*): the exact per-channel sums of squares
as Python integers, the decision on them, the mix, and the dB formula.  Nothing here calls the library.

frames are integer arrays [n, C] (int64) for the integer depths and float32 arrays [n, C] for depth 0."""
import math

import numpy as np

MIX, AUTO = -1, -2
QUIET_16 = 1073.741824                                     # (32768 * 10^(-60 / 20))^2: the -60 dBFS line as a mean square, 16-bit units
LEAD = 3.9810717055349722                                  # 10^(6 / 10): 6 dB in power


def energies(frames):
    """-> [E[c]]: the exact sum of squares of every channel, Python ints."""
    return [sum(int(v) * int(v) for v in frames[:, c].tolist()) for c in range(frames.shape[1])]


def split128(e):
    """-> (sum_lo, sum_hi) of a sum below 2^128."""
    return e & ((1 << 64) - 1), e >> 64


def as_double(e):
    """Ed = (double)sum_hi * 2^64 + (double)sum_lo, every operation rounded to nearest even as the device rounds it."""
    lo, hi = split128(e)
    return float(hi) * 18446744073709551616.0 + float(lo)


def decide(e, bits, length):
    """The channel BNHIP_CHANNEL_AUTO reads (or MIX) for a recording of `length` frames at `bits` with the sums e."""
    if len(e) == 1:
        return 0
    ed = [as_double(v) for v in e]
    quiet = (QUIET_16 * float(4 ** (bits - 16))) * float(length)
    if all(v < quiet for v in ed):
        return MIX
    top = max(range(len(ed)), key=lambda c: (ed[c], -c))
    second = max((c for c in range(len(ed)) if c != top), key=lambda c: (ed[c], -c))
    return top if ed[top] > LEAD * ed[second] else MIX


def rms_dbfs(e, bits, length):
    """computeRmsDbfs in 16-bit units from the exact sum: -96 below an rms of 1."""
    rms16 = math.sqrt(as_double(e) / float(length)) / float(1 << (bits - 16))
    return -96.0 if rms16 < 1.0 else 20.0 * math.log10(rms16 / 32768.0)


def to_float(v, bits):
    """Integer samples as the float32 the device converts them to (wav.read_wav's arithmetic)."""
    return v.astype(np.float32) / np.float32(1 << (bits - 1))


def mix(frames, bits):
    """-> float32 [n]: the mean of the channels as the device states it."""
    C = frames.shape[1]
    if bits == 0:
        acc = frames[:, 0].astype(np.float64)
        for c in range(1, C):
            acc = acc + frames[:, c].astype(np.float64)
        return (acc / np.float64(C)).astype(np.float32)
    S = frames.astype(np.int64).sum(axis=1)
    return (S.astype(np.float64) / np.float64(C * (1 << (bits - 1)))).astype(np.float32)


def pick(frames, bits, sel):
    """-> float32 [n]: what the slot launch stages for selection sel (a channel or MIX)."""
    if sel == MIX:
        return mix(frames, bits)
    return frames[:, sel].astype(np.float32) if bits == 0 else to_float(frames[:, sel], bits)


def pack(frames, bits):
    """-> the interleaved bytes of frames as a WAV data chunk holds them."""
    if bits == 0:
        return np.ascontiguousarray(frames, np.float32).tobytes()
    flat = np.ascontiguousarray(frames).reshape(-1)
    if bits == 16:
        return flat.astype("<i2").tobytes()
    w = flat.astype("<i4")
    return w.tobytes() if bits == 32 else w.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()


def go_rule(left, right):
    """recommendChannel(computeRmsDbfs(L), computeRmsDbfs(R)) (internal/audiocore/ffmpeg/analyze.go:157-202) for int16 channels, with
    math.log10: -> 0, 1 or MIX."""
    def dbfs(x):
        if len(x) == 0:
            return -96.0
        rms = math.sqrt(sum(float(int(v) * int(v)) for v in x.tolist()) / len(x))
        return -96.0 if rms < 1.0 else 20.0 * math.log10(rms / 32768.0)
    l, r = dbfs(left), dbfs(right)
    if l < -60.0 and r < -60.0:
        return MIX
    if l - r > 6.0:
        return 0
    if r - l > 6.0:
        return 1
    return MIX
