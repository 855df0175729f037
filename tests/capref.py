"""The capture bank restated in numpy (include/bnhip.h, "Capture bank"): a ring with the position clock, the write trim, the `oldest`
bound, the span rule with its five statuses and the cut - and beside it `GoCapture`, CaptureBuffer.Write / ReadSegment of
internal/audiocore/buffer/capture.go:132-179, 198-330 restated in sample positions, the wall clock replaced by the sample counter."""
import numpy as np

ALIGN = 1024
OK, CLAMPED, NOT_YET, GONE, DROPPED = 0, 1, 2, 3, 4
CLIP_SPAN = np.dtype([("start", "<i8"), ("length", "<i4"), ("recording", "<i4")])


def capacity(samples):
    return (int(samples) + ALIGN - 1) // ALIGN * ALIGN


def pcm16(data, bits):
    """Packed little-endian PCM of `bits` -> int16 as the bank stores it: clamp(rint(x * 2^15)) of the float32 x the analysis path
    reads (ties to even); a 16-bit sample as itself."""
    b = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    if bits == 16:
        return b.view("<i2").astype(np.int16)
    if bits == 24:
        t = b.reshape(-1, 3).astype(np.int32)
        v = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)
        v = np.where(v & 0x800000, v - (1 << 24), v)
        x = v.astype(np.float32) / np.float32(8388608.0)
    else:
        x = b.view("<i4").astype(np.float32) / np.float32(2147483648.0)
    y = np.rint(x.astype(np.float32) * np.float32(32768.0))              # (exact: a power of two; rint rounds ties to even)
    return np.clip(y, -32768, 32767).astype(np.int16)


class Ring:
    """One source: `cap` cells, the sample at position P of the clock in cell P mod cap."""

    def __init__(self, cap):
        self.cap, self.buf = int(cap), np.zeros(int(cap), np.int16)
        self.written = self.floor = 0

    def oldest(self):
        return max(0, self.written - self.cap, self.floor)

    def write(self, samples):
        """Every sample counts; of more than `cap` only the last `cap` are stored."""
        x = np.asarray(samples, np.int16).reshape(-1)
        keep = x[max(0, x.size - self.cap):]
        pos = self.written + x.size - keep.size + np.arange(keep.size)
        self.buf[pos % self.cap] = keep
        self.written += x.size

    def read(self, start, length):
        assert length >= 1 and self.oldest() <= start and start + length <= self.written, (start, length, self.oldest(), self.written)
        return self.buf[(start + np.arange(length)) % self.cap].copy()

    def reset(self):
        self.written = self.floor = 0


class Bank:
    def __init__(self, max_sources, capacity_samples):
        self.capacity = capacity(capacity_samples)
        self.rings = [Ring(self.capacity) for _ in range(max_sources)]

    def write(self, frames, bits=16):
        """frames [(source, bytes)]: a source's frames of one call are one write of their concatenation."""
        joined = {}
        for s, f in frames:
            joined.setdefault(s, []).append(pcm16(f, bits))
        for s, parts in joined.items():
            self.rings[s].write(np.concatenate(parts))

    def positions(self):
        return (np.array([r.written for r in self.rings], np.int64), np.array([r.oldest() for r in self.rings], np.int64))

    def valid(self, spans):
        return all(q["length"] == 0 or (0 <= q["recording"] < len(self.rings) and q["length"] > 0
                                        and self.rings[q["recording"]].oldest() <= q["start"]
                                        and q["start"] + q["length"] <= self.rings[q["recording"]].written) for q in spans)

    def read(self, spans):
        return [self.rings[int(q["recording"])].read(int(q["start"]), int(q["length"])) for q in spans if q["length"] > 0]

    def reset(self, source=-1):
        for s, r in enumerate(self.rings):
            if source < 0 or s == source:
                r.reset()


def spans(events, written, oldest, hop, pre, post, most, extended, origins=None):
    """The span rule -> (CLIP_SPAN [n], status int32 [n])."""
    out, status = np.zeros(len(events), CLIP_SPAN), np.zeros(len(events), np.int32)
    for i, e in enumerate(events):
        s = int(e["recording"])
        org = 0 if origins is None else int(origins[s])
        p0 = org + int(e["first_window"]) * hop - pre
        p1 = org + int(e["last_window"] if extended else e["first_window"]) * hop + post
        begin = max(p0, int(oldest[s]))
        out[i] = (begin, 0, s)
        if e["status"] != 0:
            status[i] = DROPPED
        elif p1 > written[s]:
            status[i] = NOT_YET
        elif begin >= p1:
            status[i] = GONE
        else:
            out[i]["length"] = min(p1, begin + most) - begin
            status[i] = CLAMPED if begin > p0 else OK
    return out, status


class GoError(Exception):
    def __init__(self, kind):
        super().__init__(kind)
        self.kind = kind


class GoCapture:
    """capture.go's CaptureBuffer of int16 samples with duration * rate == size (no alignment padding), times as sample counts.
    The reference's `now` is the capture's own progress: the samples it has counted, `total`.  start_time is the clock position of
    the buffer's first readable sample."""

    def __init__(self, size):
        self.size, self.data = int(size), np.zeros(int(size), np.int16)
        self.write_index = self.total = self.written = 0
        self.wrapped = self.initialized = False
        self.start_time = 0

    def write(self, samples):                                             # capture.go:132-179
        x = np.asarray(samples, np.int16).reshape(-1)
        if x.size == 0:
            return
        if not self.initialized:
            self.start_time, self.initialized = self.total, True
        prev = self.write_index
        if x.size > self.size:
            x = x[x.size - self.size:]                                    # only the tail is kept - and only the tail is counted
        remaining = self.size - self.write_index
        if x.size <= remaining:
            self.data[self.write_index:self.write_index + x.size] = x
        else:
            self.data[self.write_index:] = x[:remaining]
            self.data[:x.size - remaining] = x[remaining:]
        self.write_index = (self.write_index + x.size) % self.size
        self.total += x.size
        self.written = min(self.written + x.size, self.size)
        if self.write_index <= prev:
            self.wrapped = True
        if self.wrapped:
            self.start_time = self.total - self.size                      # now - bufferDuration

    def read_segment(self, start, end):                                   # capture.go:198-330
        if not self.initialized:
            raise GoError("no data")
        if not end > start:
            raise GoError("empty")
        if start < self.start_time:
            start = self.start_time
        if not end > start:
            raise GoError("empty after clamping")
        s_off, e_off = start - self.start_time, end - self.start_time
        if e_off < 0:
            raise GoError("before start")
        if e_off > self.written:
            raise GoError("insufficient")
        logical = min(self.written, self.size)
        base = (self.total - logical) % self.size if self.wrapped else 0
        si, ei = (base + s_off) % self.size, (base + e_off) % self.size
        if si == ei:
            # (extractSegment answers an empty slice here; a whole-buffer read has si == ei too, and the reference then loses it)
            return np.zeros(0, np.int16)
        if si < ei:
            return self.data[si:ei].copy()
        return np.concatenate([self.data[si:], self.data[:ei]])
