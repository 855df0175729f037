"""The audio level meter restated (include/bnhip.h, "Audio level bank"): Python integers for the sums, math.sqrt and math.log10 for
the rule, and the accumulator of the five-minute summary with its derived percentages."""
import math

import numpy as np

MAX_FRAME = 1 << 23


def scaled(sum_squares, n, clipping):
    """The rule's float64 value before the clamp and the truncation (n > 0)."""
    rms = math.sqrt(float(sum_squares) / float(n))
    db = 20 * math.log10(rms / 32768.0) if rms > 0 else -math.inf      # log10(0) = -Inf in the reference
    s = (db - (-60.0)) * (100.0 / 50.0)
    if clipping:
        s = max(s, 95.0)
    return s


def level(sum_squares, n, clipping):
    if n == 0:
        return 0
    s = scaled(sum_squares, n, clipping)
    s = 0.0 if s < 0 else 100.0 if s > 100 else s
    return int(s)


def measure(q):
    """int16 samples -> (sum of squares, full-scale samples, level, clipping) with exact integers."""
    q = np.asarray(q, np.int16).astype(np.int64)
    total = int((q * q).sum(dtype=np.int64))                           # exact: at most 2^23 squares of at most 2^30
    clipped = int(((q == 32767) | (q == -32768)).sum())
    return total, clipped, level(total, q.size, clipped > 0), clipped > 0


def pcm16_of(raw, bits):
    """sample_pcm16(frame_sample<bits>) restated: packed little-endian PCM bytes -> the int16 the meter measures and the capture
    ring stores.  float32 throughout, as the kernels: x = v / 2^(bits-1) (int32 -> float32 rounds to nearest even first), then
    clamp(rint(x * 32768), -32768, 32767)."""
    b = np.frombuffer(bytes(raw), np.uint8)
    if bits == 16:
        return b.view("<i2").copy()
    if bits == 24:
        t = b.reshape(-1, 3).astype(np.int32)
        v = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)
        v = np.where(v & 0x800000, v - (1 << 24), v).astype(np.int32)
        x = v.astype(np.float32) / np.float32(8388608.0)
    else:
        x = b.view("<i4").astype(np.float32) / np.float32(2147483648.0)
    y = np.rint(x * np.float32(32768.0))
    return np.clip(y, -32768.0, 32767.0).astype(np.int16)


class Stats:
    """audioLevelAccum (audio_level_stats.go:14-73) and logAndReset's derived fields (:114-120)."""

    def __init__(self):
        self.sum = self.count = self.zero_count = self.clip_count = 0
        self.min = self.max = 0

    def record(self, level, clipping):
        if self.count == 0:
            self.min = self.max = level
        else:
            self.min, self.max = min(self.min, level), max(self.max, level)
        self.sum += level
        self.count += 1
        self.zero_count += level == 0
        self.clip_count += bool(clipping)

    def fields(self):
        d = dict(sum=self.sum, count=self.count, zero_count=self.zero_count, clip_count=self.clip_count, min=self.min, max=self.max,
                 avg_level=0, zero_pct=0, clipping_pct=0)
        if self.count:
            d.update(avg_level=self.sum // self.count, zero_pct=self.zero_count * 100 // self.count,
                     clipping_pct=self.clip_count * 100 // self.count)
        return d
