"""Real-time window path either side of the device call, host side.

  a3  `AnalysisBuffer`      internal/audiocore/buffer/analysis.go:30-273 (+ overwrite.go)     ring -> `overlap ‖ fresh` windows
  a4  `process_data`        internal/analysis/process.go:253-422 (+ :44-213 overrun tracker)   convert -> predict -> overrun -> enqueue
  a5  `Orchestrator`        internal/classifier/orchestrator.go:63-68,514-572                  lock protocol + counters
      `ModelSpec`           internal/classifier/model.go:33-56                                  window geometry (50 % overlap)
      `BufferMonitor.tick`  internal/analysis/buffer_manager.go:388-496                         one poll of one (source, model)

The reference runs one window at a time: every (source, model) pair has its own 100 ms poll loop and all of them queue on
`inferenceMu` for a batch-1 native call.  `WindowBatcher` is the same contract turned the way the GPU wants it: one tick reads
every buffer that has a window ready and hands all of them to ONE device call (PCM bytes go to the device as they are - the
16/24/32-bit conversion of a1 happens in the kernel), then builds one `Results` message per window.  Per-window semantics
(copy of the PCM bytes, overrun accounting against the model's buffer interval, drop-on-full queue) are the reference's.

Two holders of the rings: `AnalysisBuffer` below mirrors the reference's type one to one (its tests are the reference's
table); `NativeWindows` is the library's window assembler behind the C ABI (`bnhip_windows_*`, csrc/windows.cpp) - the form a
Go host binds - which reads every ready source into consecutive rows of one page-locked batch buffer, so that the device call
copies the windows from where they were assembled.  `WindowBatcher` uses the native one unless told otherwise; both are held
to the same oracle.

Byte work here is exact by construction (numpy slices); tests/test_stream.py replays the reference's own table of cases
(analysis_test.go:23-243) and compares against the line-by-line restatement in oracle/gostream.py.
"""
import ctypes as C
import math
import threading
import time
from dataclasses import dataclass

import numpy as np

from . import host as _host
from . import results as _results

# analysis.go:13-18
OVERWRITE_WINDOW_S = 5 * 60.0
OVERWRITE_RATE_THRESHOLD = 10
OVERWRITE_MIN_WRITES = 50
OVERWRITE_NOTIFY_COOLDOWN_S = 3600.0
# process.go:34-40
OVERRUN_REPORT_COOLDOWN_S = 3600.0
OVERRUN_MIN_COUNT = 10
NUM_CHANNELS, BYTES_PER_SAMPLE = 1, 2        # conf.NumChannels, conf.BytesPerSample (16-bit capture)


class StreamError(ValueError):
    """Validation failure (the reference's errors.CategoryValidation)."""


def _as_bytes(data):
    """bytes-like or ndarray of any dtype / layout -> flat uint8 view (a copy only when the array is not contiguous)."""
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data).reshape(-1).view(np.uint8)
    return np.frombuffer(data, np.uint8)


class ByteRing:
    """Byte ring in overwrite mode.  The reference uses github.com/smallnest/ringbuffer v0.1.1 (go.mod:31, absent from the
    snapshot) with `SetOverwrite(true)` (analysis.go:120): a write never fails, the oldest unread bytes are dropped when the
    data does not fit, and of a write longer than the ring only the last `capacity` bytes survive."""

    def __init__(self, capacity):
        self.buf = np.zeros(capacity, np.uint8)
        self.cap, self.r, self.n = capacity, 0, 0          # read position, unread byte count

    def length(self):
        return self.n

    def free(self):
        return self.cap - self.n

    def write(self, data):
        d = _as_bytes(data)
        total = d.size
        if total > self.cap:                                # only the newest `cap` bytes can survive
            drop = total - self.cap
            d = d[drop:]
            self.r, self.n = (self.r + self.n) % self.cap, 0   # everything unread is older than what is kept
        over = d.size - self.free()
        if over > 0:                                        # advance the read position past the bytes being overwritten
            self.r = (self.r + over) % self.cap
            self.n -= over
        w = (self.r + self.n) % self.cap
        first = min(d.size, self.cap - w)
        self.buf[w:w + first] = d[:first]
        self.buf[:d.size - first] = d[first:]
        self.n += d.size
        return total

    def read_into(self, out):
        """Fills `out` with up to len(out) unread bytes; returns the count (ring.Read)."""
        n = min(out.size, self.n)
        first = min(n, self.cap - self.r)
        out[:first] = self.buf[self.r:self.r + first]
        out[first:n] = self.buf[:n - first]
        self.r = (self.r + n) % self.cap
        self.n -= n
        return n

    def reset(self):
        self.r = self.n = 0


class OverwriteTracker:
    """overwrite.go: writes / overwrites within a sliding window, a warning when the rate passes the threshold."""

    def __init__(self, window_s=OVERWRITE_WINDOW_S, rate_threshold=OVERWRITE_RATE_THRESHOLD, min_writes=OVERWRITE_MIN_WRITES,
                 notify_cooldown_s=OVERWRITE_NOTIFY_COOLDOWN_S, on_warn=None, clock=time.monotonic):
        self.mu = threading.Lock()
        self.total_writes = self.overwrite_count = 0
        self.clock = clock
        self.window_start, self.last_notified = clock(), None
        self.window_s, self.rate_threshold, self.min_writes, self.cooldown = window_s, rate_threshold, min_writes, notify_cooldown_s
        self.on_warn = on_warn

    def record_write(self):
        with self.mu:
            if self.window_s > 0 and self.clock() - self.window_start > self.window_s:
                self.total_writes = self.overwrite_count = 0
                self.window_start = self.clock()
            self.total_writes += 1

    def record_overwrite(self):
        with self.mu:
            self.overwrite_count += 1

    def check_and_notify(self, source_id):
        with self.mu:
            if self.total_writes == 0 or self.total_writes < self.min_writes:
                return False
            rate = self.overwrite_count / self.total_writes * 100
            if int(rate) < self.rate_threshold:
                return False
            now = self.clock()
            if self.cooldown > 0 and self.last_notified is not None and now - self.last_notified < self.cooldown:
                return False
            self.last_notified = now
            writes, overwrites = self.total_writes, self.overwrite_count
        if self.on_warn:                                  # outside the lock: the callback may look at the tracker
            self.on_warn(source_id, rate, writes, overwrites)
        return True

    def overwrite_rate(self):
        with self.mu:
            return 0.0 if self.total_writes == 0 else self.overwrite_count / self.total_writes * 100

    def reset(self):
        with self.mu:
            self.total_writes = self.overwrite_count = 0
            self.window_start = self.clock()


class AnalysisBuffer:
    """analysis.go: each `read` returns `overlap_size` bytes kept from the end of the previous window followed by
    `read_size` fresh bytes; the very first window's prefix is zeros; `None` = try again later."""

    def __init__(self, capacity, overlap_size, read_size, source_id, on_warn=None):
        if capacity <= 0:
            raise StreamError(f"invalid analysis buffer capacity: {capacity}, must be greater than 0")
        if overlap_size < 0:
            raise StreamError(f"invalid overlap size: {overlap_size}, must be >= 0")
        if read_size <= 0:
            raise StreamError(f"invalid read size: {read_size}, must be greater than 0")
        if read_size < overlap_size:
            raise StreamError(f"read size {read_size} must be >= overlap size {overlap_size}")
        if capacity < read_size:
            raise StreamError(f"capacity {capacity} must be >= read size {read_size}")
        if not source_id:
            raise StreamError("source ID must not be empty")
        self.ring = ByteRing(capacity)
        self.prev = None
        self.overlap_size, self.read_size, self.window_size = overlap_size, read_size, overlap_size + read_size
        self.source_id = source_id
        self.tracker = OverwriteTracker(on_warn=on_warn)
        self.mu = threading.Lock()

    def write(self, data):
        d = _as_bytes(data)
        with self.mu:
            will_overwrite = d.size > self.ring.free()
            self.ring.write(d)
        self.tracker.record_write()
        if will_overwrite:
            self.tracker.record_overwrite()
        self.tracker.check_and_notify(self.source_id)

    def ready(self):
        with self.mu:
            return self.ring.length() >= self.read_size

    def read(self, out=None):
        """-> uint8[window_size] (a fresh array, or `out` filled), or None when fewer than read_size bytes are buffered."""
        with self.mu:
            if self.ring.length() < self.read_size:
                return None
            win = out if out is not None else np.empty(self.window_size, np.uint8)
            ov = self.overlap_size
            if ov > 0:
                if self.prev is not None and self.prev.size == ov:
                    win[:ov] = self.prev
                else:
                    win[:ov] = 0
            n = self.ring.read_into(win[ov:ov + self.read_size])
            if n < self.read_size:
                win[ov + n:] = 0
            if ov > 0:
                if self.prev is None:
                    self.prev = np.zeros(ov, np.uint8)
                fresh_end = ov + n
                if n >= ov:
                    self.prev[:] = win[fresh_end - ov:fresh_end]
                else:
                    self.prev[:] = 0
                    self.prev[ov - n:] = win[ov:fresh_end]
            return win

    def overwrite_count(self):
        with self.tracker.mu:
            return self.tracker.overwrite_count

    def reset(self):
        with self.mu:
            self.ring.reset()
            self.prev = None
        self.tracker.reset()


class NativeWindows:
    """`bnhip_windows` (include/bnhip.h): per-source rings + overlap tails in the library, every ready window collected into one
    batch buffer (page-locked when a device is present).  One assembler per window geometry, i.e. per model."""

    _proto_done = False

    def __init__(self, overlap_bytes, read_bytes, max_batch=256):
        lib = self._lib = _host.load_library()
        if not NativeWindows._proto_done:
            vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
            lib.bnhip_windows_create.argtypes = [sz, sz, ci, C.POINTER(vp)]
            lib.bnhip_windows_info.argtypes = [vp, C.POINTER(sz), C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
            lib.bnhip_windows_add_source.argtypes = [vp, C.c_char_p, sz, C.POINTER(ci)]
            lib.bnhip_windows_remove_source.argtypes = [vp, ci]
            lib.bnhip_windows_write.argtypes = [vp, ci, vp, sz]
            lib.bnhip_windows_collect.argtypes = [vp, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(vp)]
            lib.bnhip_windows_ready.argtypes = [vp, C.POINTER(ci)]
            lib.bnhip_windows_stats.argtypes = [vp, ci, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(sz)]
            lib.bnhip_windows_reset.argtypes = [vp, ci]
            lib.bnhip_windows_destroy.argtypes = [vp]
            lib.bnhip_windows_predict_topk.argtypes = [vp, vp, ci, ci, C.c_double, ci, C.POINTER(ci), C.POINTER(ci), vp, vp,
                                                       C.POINTER(vp)]
            lib.bnhip_windows_destroy.restype = None
            NativeWindows._proto_done = True
        if overlap_bytes < 0 or read_bytes < 0:
            raise StreamError(f"invalid window geometry: overlap {overlap_bytes}, read {read_bytes}")
        h = C.c_void_p()
        self._h = None
        self._check(lib.bnhip_windows_create(overlap_bytes, read_bytes, max_batch, C.byref(h)))
        self._h = h
        wb, mb, pin = C.c_size_t(), C.c_int(), C.c_int()
        self._check(lib.bnhip_windows_info(h, C.byref(wb), C.byref(mb), C.byref(pin), None))
        self.window_bytes, self.max_batch, self.pinned = wb.value, mb.value, bool(pin.value)
        self.overlap_size, self.read_size = overlap_bytes, read_bytes
        self._sources = (C.c_int * self.max_batch)()
        self._rows = None                               # uint8 [max_batch, window_bytes] over the library's batch buffer

    def _check(self, rc):
        if rc != _host.BNHIP_OK:
            msg = (self._lib.bnhip_last_error() or b"").decode("utf-8", "replace")
            if rc == _host.E_INVALID:
                raise StreamError(msg)
            raise _host.HipError(rc, msg)

    def _alive(self):
        if self._h is None:
            raise StreamError("window assembler is closed")
        return self._h

    def add_source(self, source_id, capacity):
        idx = C.c_int(-1)
        self._check(self._lib.bnhip_windows_add_source(self._alive(), source_id.encode(), max(0, capacity), C.byref(idx)))
        return idx.value

    def remove_source(self, source):
        self._check(self._lib.bnhip_windows_remove_source(self._alive(), source))

    def write(self, source, data):
        d = _as_bytes(data)
        self._check(self._lib.bnhip_windows_write(self._alive(), source, d.ctypes.data, d.size))

    def collect(self, cap=None):
        """-> (source indices, uint8 [n, window_bytes] VIEW of the batch buffer, valid until the next collect)."""
        n, p = C.c_int(0), C.c_void_p()
        cap = self.max_batch if cap is None else min(cap, self.max_batch)
        self._check(self._lib.bnhip_windows_collect(self._alive(), cap, self._sources, C.byref(n), C.byref(p)))
        return list(self._sources[:n.value]), self._view(p)[:n.value]

    def _view(self, p):
        if self._rows is None:
            buf = (C.c_uint8 * (self.max_batch * self.window_bytes)).from_address(p.value)
            self._rows = np.frombuffer(buf, np.uint8).reshape(self.max_batch, self.window_bytes)
        return self._rows

    def predict_topk(self, clf, bit_depth=16, k=10, activation=0, sensitivity=1.0):
        """collect + device call in one (bnhip_windows_predict_topk): the rows of chunk c + 1 are assembled while chunk c is on
        the device.  clf: host.HipClassifier.  -> (source indices, rows view, conf [n, kk], idx [n, kk]); on a device error the
        exception carries `.sources` - those windows are consumed all the same."""
        clf._alive()
        kk = min(k, clf.num_species())
        if getattr(self, "_tk", None) is None or self._tk[0].shape[1] != kk:
            self._tk = (np.empty((self.max_batch, kk), np.float32), np.empty((self.max_batch, kk), np.int32))
        conf, idx = self._tk
        n, p = C.c_int(0), C.c_void_p()
        rc = self._lib.bnhip_windows_predict_topk(self._alive(), clf._h, bit_depth, activation, sensitivity, k, self._sources,
                                                  C.byref(n), conf.ctypes.data, idx.ctypes.data, C.byref(p))
        srcs = list(self._sources[:n.value])
        if rc != _host.BNHIP_OK:
            try:
                self._check(rc)
            except Exception as e:
                e.sources = srcs
                raise
        return srcs, self._view(p)[:n.value], conf[:n.value].copy(), idx[:n.value].copy()

    def predict_events(self, clf, bank, bit_depth=16, k=10, activation=0, sensitivity=1.0):
        """predict_topk with the tick's rows also fed to `bank` (host.EventBank) behind the last chunk, in the same call
        (bnhip_windows_predict_events).  -> (source indices, rows view, conf, idx, the events that became due).  A tick whose
        events do not fit the room feeds the bank the returned rows instead: the refused call has changed no source."""
        clf._alive()
        lib = _host._event_bank_protos(self._lib)
        kk = min(k, clf.num_species())
        if getattr(self, "_tk", None) is None or self._tk[0].shape[1] != kk:
            self._tk = (np.empty((self.max_batch, kk), np.float32), np.empty((self.max_batch, kk), np.int32))
        conf, idx = self._tk
        if getattr(self, "_ev", None) is None:
            self._ev = np.zeros(4096, _host.EVENT)
        n, p, ne = C.c_int(0), C.c_void_p(), C.c_size_t(0)
        rc = lib.bnhip_windows_predict_events(self._alive(), clf._h, bank._alive(), bit_depth, activation, sensitivity, k, self._sources,
                                              C.byref(n), conf.ctypes.data, idx.ctypes.data, C.byref(p), self._ev.ctypes.data, self._ev.size,
                                              C.byref(ne))
        srcs = list(self._sources[:n.value])
        events = None
        if rc == _host.E_INVALID and ne.value > self._ev.size:
            events, rc = bank.process(srcs, conf[:n.value], idx[:n.value]), _host.BNHIP_OK
        if rc != _host.BNHIP_OK:
            try:
                self._check(rc)
            except Exception as e:
                e.sources = srcs
                raise
        if events is None:
            events = self._ev[:ne.value].copy()
            if bank.dynamic and n.value:                            # (the bank's call ran: its change records join the bank's list)
                bank._collect_changes()
        return srcs, self._view(p)[:n.value], conf[:n.value].copy(), idx[:n.value].copy(), events

    def ready(self):
        n = C.c_int(0)
        self._check(self._lib.bnhip_windows_ready(self._alive(), C.byref(n)))
        return n.value

    def stats(self, source):
        w, o, b = C.c_uint64(), C.c_uint64(), C.c_size_t()
        self._check(self._lib.bnhip_windows_stats(self._alive(), source, C.byref(w), C.byref(o), C.byref(b)))
        return w.value, o.value, b.value

    def reset(self, source):
        self._check(self._lib.bnhip_windows_reset(self._alive(), source))

    def close(self):
        if self._h is not None:
            self._rows = None
            self._lib.bnhip_windows_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _NativeSource:
    """One source of a NativeWindows with the AnalysisBuffer's surface (write / ready / overwrite_count / reset)."""

    def __init__(self, win: NativeWindows, index, source_id, model_id=None):
        self.win, self.index, self.source_id, self.model_id = win, index, source_id, model_id
        self.read_size, self.overlap_size, self.window_size = win.read_size, win.overlap_size, win.window_bytes

    def write(self, data):
        self.win.write(self.index, data)

    def ready(self):
        return self.win.stats(self.index)[2] >= self.read_size

    def overwrite_count(self):
        return self.win.stats(self.index)[1]

    def reset(self):
        self.win.reset(self.index)


@dataclass(frozen=True)
class ModelSpec:
    """model.go:33-56.  `sample_rate` is what the window is sized by; `raw_sample_rate` what the model is fed at."""
    sample_rate: int
    clip_length_s: float
    raw_sample_rate: int = 0
    clip_bytes: int = 0            # test geometries whose clip is not a whole number of seconds; 0 = the reference's formula

    def clip_size_bytes(self):
        if self.clip_bytes:
            return self.clip_bytes
        return self.sample_rate * int(self.clip_length_s) * NUM_CHANNELS * BYTES_PER_SAMPLE

    def buffer_dimensions(self):
        clip = self.clip_size_bytes()
        overlap = clip // 2
        return clip, overlap, clip - overlap

    def buffer_interval_s(self):
        return self.clip_length_s / 2

    def effective_sample_rate(self):
        return self.raw_sample_rate if self.raw_sample_rate > 0 else self.sample_rate


class OverrunTrackers:
    """process.go:44-213: per (source, model) tumbling one-hour window of "inference took longer than the buffer interval"."""

    class _T:
        __slots__ = ("mu", "source", "model_id", "count", "window_start", "max_elapsed", "buffer_len")

        def __init__(self, source, model_id):
            self.mu = threading.Lock()
            self.source, self.model_id = source, model_id
            self.count, self.window_start, self.max_elapsed, self.buffer_len = 0, None, 0.0, 0.0

    def __init__(self, on_report=None, clock=time.monotonic):
        self.mu = threading.Lock()
        self.m = {}
        self.on_report, self.clock = on_report, clock

    def get(self, source, model_id):
        key = source + ":" + model_id
        with self.mu:
            t = self.m.get(key)
            if t is None:
                t = self.m[key] = self._T(source, model_id)
            return t

    def record(self, source, model_id, elapsed_s, buffer_len_s):
        t = self.get(source, model_id)
        with t.mu:
            now = self.clock()
            if t.window_start is None:
                t.window_start = now
            if now - t.window_start >= OVERRUN_REPORT_COOLDOWN_S:
                if t.count >= OVERRUN_MIN_COUNT and self.on_report:
                    self.on_report(t.source, t.model_id, t.count, t.max_elapsed, t.buffer_len, now - t.window_start)
                t.count, t.max_elapsed, t.window_start = 0, 0.0, now
            t.count += 1
            if elapsed_s > t.max_elapsed:
                t.max_elapsed, t.buffer_len = elapsed_s, buffer_len_s

    def count(self, source, model_id):
        t = self.get(source, model_id)
        with t.mu:
            return t.count

    def remove_source(self, source):
        with self.mu:
            for k in [k for k in self.m if k.startswith(source + ":")]:
                del self.m[k]

    def cleanup(self, max_age_s):
        now = self.clock()
        with self.mu:
            for k, t in list(self.m.items()):
                with t.mu:
                    idle = t.window_start is not None and now - t.window_start > max_age_s
                    nothing = t.window_start is None and t.count == 0
                if idle or nothing:
                    del self.m[k]

    def reset(self):
        with self.mu:
            self.m.clear()


class OrchestratorError(RuntimeError):
    pass


class Orchestrator:
    """orchestrator.go:63-68,514-572.  Lock order: models map -> `inference_mu` (one native call at a time, whatever the model)
    -> the entry's own lock (instance lifecycle).  The map lock is dropped before the other two are taken so that unloading a
    model never waits behind an inference.  An instance is anything with `predict_batch(flat, n)` (host.BirdNET / Perch)."""

    class _Entry:
        def __init__(self, instance, spec):
            self.mu = threading.Lock()
            self.instance, self.spec, self.active = instance, spec, True

    def __init__(self, counters: _results.CounterMap = None):
        self.mu = threading.Lock()
        self.inference_mu = threading.Lock()
        self.models = {}
        self.counters = counters if counters is not None else _results.CounterMap()

    def register(self, model_id, instance, spec: ModelSpec):
        with self.mu:
            self.models[model_id] = self._Entry(instance, spec)

    def unload(self, model_id):
        """Takes the map lock and the entry lock but NOT `inference_mu` (orchestrator.go:66)."""
        with self.mu:
            e = self.models.pop(model_id, None)
        if e is not None:
            with e.mu:
                inst, e.instance = e.instance, None
            if inst is not None and hasattr(inst, "close"):
                inst.close()
            self.counters.delete(model_id)

    def model_spec_for(self, model_id):
        with self.mu:
            e = self.models.get(model_id)
        return e.spec if e is not None else None

    def set_active(self, model_id, on):
        with self.mu:
            e = self.models.get(model_id)
        if e is not None:
            e.active = bool(on)

    def is_model_active(self, model_id):
        with self.mu:
            e = self.models.get(model_id)
        return e is not None and e.active

    def predict_model(self, model_id, call):
        """`call(instance)` runs under the three locks; its duration goes to the per-model counters, an exception to the
        error counter (PredictModel :553-569)."""
        with self.mu:
            e = self.models.get(model_id)
        if e is None:
            raise OrchestratorError(f"unknown model: {model_id}")
        with self.inference_mu:
            with e.mu:
                if e.instance is None:
                    raise OrchestratorError(f"model {model_id} has been closed")
                t0 = time.perf_counter()
                try:
                    out = call(e.instance)
                except Exception:
                    self.counters.record_error(model_id)
                    raise
                self.counters.record_invoke(model_id, (time.perf_counter() - t0) * 1e6)
                return out


def _pcm_windows_predict(instance, windows, bit_depth):
    """windows uint8 [n, window_bytes] -> per-window top-K lists.  The bytes go to the device as they are when the instance
    can take them (`predict_pcm_batch`); otherwise they are widened here with the reference's own arithmetic (a1)."""
    n = windows.shape[0]
    if hasattr(instance, "predict_pcm_batch"):
        return instance.predict_pcm_batch(windows.reshape(-1), bit_depth, n)
    if bit_depth == 16:
        x = windows.reshape(-1).view("<i2").astype(np.float32) / np.float32(32768.0)
    elif bit_depth == 32:
        x = windows.reshape(-1).view("<i4").astype(np.float32) / np.float32(2147483648.0)
    elif bit_depth == 24:
        b = windows.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v & 0x800000, v - (1 << 24), v)
        x = v.astype(np.float32) / np.float32(8388608.0)
    else:
        raise StreamError(f"unsupported audio bit depth: {bit_depth}")
    return instance.predict_batch(x, n)


def process_windows(orch: Orchestrator, windows, start_times, captured_at, sources, model_id, queue: _results.ResultsQueue,
                    overruns: OverrunTrackers, bit_depth=16, threshold=0.0):
    """`ProcessData` for n windows of one model at once.  Returns the number of messages enqueued.
    Elapsed time, the overrun check and the queue message are per window as in process.go:327-420; the one difference is
    that the n windows share one device call, so each window's elapsed time is the whole call's (what a consumer waiting
    for that window actually saw)."""
    windows = np.ascontiguousarray(windows, np.uint8)
    if windows.ndim == 1:
        windows = windows[None]
    t0 = time.perf_counter()
    lists = orch.predict_model(model_id, lambda inst: _pcm_windows_predict(inst, windows, bit_depth))
    elapsed = time.perf_counter() - t0
    return _emit_results(orch, windows, lists, elapsed, start_times, captured_at, sources, model_id, queue, overruns, threshold)


def _emit_results(orch, windows, lists, elapsed, start_times, captured_at, sources, model_id, queue, overruns, threshold=0.0):
    """ProcessData's tail per window (process.go:327-420): overrun check, PCM copy, enqueue-or-drop.  sources[i] None = skip."""
    spec = orch.model_spec_for(model_id)
    interval = spec.buffer_interval_s() if spec is not None else 1.5       # fallback: BirdNET v2.4 (process.go:353)
    sent = 0
    for i in range(windows.shape[0]):
        if sources[i] is None:
            continue
        if elapsed > interval:
            overruns.record(sources[i], model_id, elapsed, interval)
        dets = [_results.Detection(lbl, conf) for lbl, conf in lists[i] if conf >= threshold]
        msg = _results.Results(start_time=float(start_times[i]), audio_captured_at=float(captured_at[i]),
                               pcm_data=windows[i].tobytes(),            # independent copy: the window goes back to its pool
                               results=dets, elapsed_time=elapsed, source=sources[i], model_id=model_id)
        sent += queue.offer(msg)
    return sent


def process_data(orch, data, start_time, captured_at, source, model_id, queue, overruns, bit_depth=16):
    """The reference's signature: one window."""
    return process_windows(orch, np.frombuffer(data, np.uint8)[None], [start_time], [captured_at], [source], model_id, queue,
                           overruns, bit_depth)


@dataclass(frozen=True)
class CaptureSettings:
    """WindowBatcher(capture=...): every source's last `seconds` of audio stay on the device (one host.CaptureBank per model, at
    the model's rate, max_sources rings: max_sources * seconds * rate * 2 bytes) and every approved detection event is answered with
    its clip, cut, normalised, FLAC-encoded and rendered there under `export` (a wav.ClipExport).  Under extended capture
    (WindowBatcher(extend=...), export.extended) an event is answered only once its deadline has passed, up to the extend's
    max_seconds behind its first hit: `seconds` must then hold max_seconds plus the pre-capture (and the ticks until the export),
    or the head of a long event has left the ring by the time it is due and the event is reported without a clip."""
    seconds: float
    export: object
    max_sources: int = 256


class WindowBatcher:
    """All (source, model) monitors of buffer_manager.go:388-496 in one object.  `tick()` is one poll: every buffer with a
    window ready is read, windows of the same model form one batch (at most `max_batch` per device call), inactive models
    are read and discarded exactly as the reference does (:478-480: the audio is consumed, not analysed).

    A buffer allocated with a `source_rate` other than its model's effective rate is fed resampled audio, BufferConsumer.Write's
    rate groups (buffer_consumer.go:105-210): a source's buffers are grouped by (source rate, model rate) and each group's
    audio is resampled once per frame, whatever the number of models in it.  Python rings: one host.StreamResampler per
    (source, rate pair), then one buffer write per frame, as the reference.  Native rings: the frames are queued per rate pair
    and the next `tick()` resamples every source's queued frames in ONE device call per rate pair (host.ResamplerBank, one
    ring write per frame) before it collects - such a buffer's audio therefore reaches its ring up to one tick later than
    audio at the model's own rate.

    `set_processing(source, source_rate, filters, gain_db)` gives a source the analysis route's EQ chain and input gain
    (AudioRouter.applyProcessing, internal/audiocore/router.go:1006-1080): every frame of the source is converted to float64,
    filtered, scaled, clamped and truncated back to PCM16 once, at the source rate, before the rate grouping above, so every
    buffer of the source, resampled or not, sees the processed bytes.  A source without filters and with 0 dB gain is not
    processed at all (router.go:848).  Python rings: one host.EqualizerBank call per write.  Native rings: a processed
    source's frames are queued in order and the next `tick()` processes every source's queued frames in ONE device call,
    then writes them to the source's rings (straight from the library when each frame has one ring at the model's rate and all
    of them are in one assembler) and into the same tick's resampler queue, before it collects - a processed source's audio
    therefore reaches its rings up to one tick late, as resampled audio does.  A failed call costs its own frames only
    (on_error), as the reference drops a frame whose processing failed.

    `set_sound_level(source, source_rate, interval_s)` gives a source the 1/3-octave sound level monitor (soundlevel.Processor
    behind a SoundLevelConsumer route, internal/analysis/audio_pipeline_service.go:685-740): every frame of the source, at the
    source rate and after set_processing's EQ and gain, is one ProcessSamples call, and `take_sound_levels()` returns the
    finished SoundLevelData-shaped reports.  One host.SoundLevelBank per source rate.  Python rings: one bank call per write.
    Native rings: the frames are queued and the next `tick()` runs one bank call per rate, after the EQ drain and before the
    resampler drain.  A failed call costs its own frames only (on_error), as the consumer logs the error and goes on.

    `set_audio_level(source)` gives a source the input level meter (calculateAudioLevel behind an AudioLevelConsumer route,
    internal/analysis/audio_level_consumer.go:65-93): every frame given to write(source, data) is one measurement, of the frame as
    given - at the source's rate and BEFORE set_processing's EQ and gain, as the reference's level consumer is a route of its own
    beside the analysis route - and `take_audio_levels()` returns the AudioLevelData-shaped results.  One host.LevelBank for all
    sources.  Python rings: one bank call per write.  Native rings: the frames are queued and the next `tick()` measures every
    source's queued frames in one bank call, ahead of the EQ drain.  A failed call costs its own frames only (on_error).
    `audio_level_stats(source, reset)` answers the source's five-minute-summary accumulators.

    `events=` (a host.EventTables) adds the detection events of every tick (take_events, on_events).  With `capture=` (a
    CaptureSettings; native rings, with events) the bytes that reach a source's ring are also staged for the model's
    host.CaptureBank: a tick uploads them in one write call before the model call, and the events that became due are answered
    with their clips in one export call (take_clips, on_clips).  An event whose clip ends behind what has been written is kept and
    tried again on later ticks, never cut short; one whose audio has left the ring is reported without a clip.

    `extend=` (a host.EventExtend; native rings, with events) creates every model's event bank extended: the hits of the chosen classes move their
    events' deadlines (include/bnhip.h, "Detection events: extended capture"), so a bird that keeps calling is one long event.  With
    `capture=` and an export with extended=True such an event's clip runs from its first hit to its last; the retry above waits for
    the audio behind the last hit.

    `dynamic=` (a host.EventDynamic; native rings, with events) creates every model's event bank dynamic: the bank learns per-class
    thresholds on the device (include/bnhip.h, "Detection events: dynamic thresholds"; one bank per model is the reference's
    modelID:species scoping).  Bank time is the batcher's `clock` in milliseconds since its creation, set before every tick; the
    EventDynamic's valid and cooldown are in that unit.  The ticks' threshold changes go to take_threshold_changes() and
    on_threshold_changes(model_id, changes).

    `guards=` (a host.EventGuards; native rings, with events) sets the dog-bark and daylight filters on every model's event bank
    (include/bnhip.h, "Detection events: dog-bark and daylight filters"): an event that the reference's flush would discard for a
    recent dog bark or for beginning in daylight carries status host.EVENT_DOG or host.EVENT_DAYLIGHT and, without
    EVENTS_KEEP_DROPPED, is not answered - nor learnt from, nor cut.  `set_guards(guards | None)` changes them from the next tick
    on, `set_daylight(source, intervals)` gives a source its daylight intervals."""

    BANK_STREAMS = 1024                      # native: streams per rate pair's resampler bank
    EVENT_SOURCES = 1024                     # native: sources of a model's event bank (assembler slots are reused)

    def __init__(self, orch: Orchestrator, queue: _results.ResultsQueue = None, overruns: OverrunTrackers = None,
                 max_batch=256, pre_capture_s=0.0, bit_depth=16, clock=time.time, on_error=None, native=True, events=None,
                 on_events=None, capture=None, on_clips=None, extend=None, dynamic=None, on_threshold_changes=None, guards=None):
        if capture is not None and (events is None or not native):
            raise StreamError("capture needs events and the native rings")
        if extend is not None and (events is None or not native):
            raise StreamError("extend needs events and the native rings")
        if dynamic is not None and (events is None or not native):
            raise StreamError("dynamic needs events and the native rings")
        if guards is not None and (events is None or not native):
            raise StreamError("guards need events and the native rings")
        self.orch = orch
        self.queue = queue if queue is not None else _results.ResultsQueue()
        self.overruns = overruns if overruns is not None else OverrunTrackers()
        self.max_batch, self.pre_capture_s, self.bit_depth, self.clock = max_batch, pre_capture_s, bit_depth, clock
        self.buffers = {}                    # (source, model_id) -> AnalysisBuffer | _NativeSource
        self.native = native                 # rings in the library, windows collected into its page-locked batch buffer
        self.assemblers = {}                 # native: model_id -> NativeWindows
        self.mu = threading.Lock()
        self.on_error, self.errors = on_error, 0   # a failed device call costs its own windows only (the reference logs and polls on)
        self.rates = {}                      # (source, model_id) -> (source rate, model rate) of a resampled buffer
        self.resamplers = {}                 # python: (source, source rate, model rate) -> host.StreamResampler
        self.banks = {}                      # native: (source rate, model rate) -> host.ResamplerBank
        self.bank_streams = {}               # native: (source, source rate, model rate) -> stream of that pair's bank
        self.pending = {}                    # native: (source rate, model rate) -> [(source, stream, pcm bytes, buffers)] until the next tick
        self.eq_bank = None                  # host.EqualizerBank of the processed sources (created on first use)
        self.eq_streams = {}                 # source -> its stream of eq_bank
        self.eq_pending = []                 # native: [(source, stream, pcm bytes)] of processed sources until the next tick
        self.sl_banks = {}                   # source rate -> host.SoundLevelBank (created on first use)
        self.sl_streams = {}                 # source -> (source rate, stream of that rate's bank, name)
        self.sl_pending = {}                 # native: source rate -> [(source, stream, pcm bytes)] until the next tick
        self.sl_reports = []                 # finished reports until take_sound_levels()
        self.al_bank = None                  # host.LevelBank of the metered sources (created on first use)
        self.al_streams = {}                 # source -> (its stream of al_bank, name)
        self.al_pending = []                 # native: [(source, stream, pcm bytes)] of metered sources until the next tick
        self.al_reports = []                 # measurements until take_audio_levels()
        self.events = events                 # native: a host.EventTables -> detection events beside the Results (None: none)
        self.extend = extend                 # native: a host.EventExtend -> the models' event banks are created extended (None: not)
        self.dynamic = dynamic               # native: a host.EventDynamic -> the models' event banks learn their thresholds (None: not)
        self.guards = guards                 # native: a host.EventGuards -> set on the models' event banks (None: none)
        self.daylight = {}                   # (model_id, assembler source) -> [(from, to)] in windows, for the bank of that model
        self.on_threshold_changes = on_threshold_changes
        self.threshold_reports = []          # the ticks' threshold changes until take_threshold_changes()
        self.created, self.bank_now = clock() if dynamic is not None else None, 0   # bank time: milliseconds of `clock` since here, never decreasing
        self.on_events = on_events
        self.event_banks = {}                # native: model_id -> host.EventBank over that model's assembler sources
        self.event_reports = []              # the ticks' events until take_events()
        self.capture = capture               # native: a CaptureSettings -> the events' clips from per-source rings on the device
        self.on_clips = on_clips
        self.capture_banks = {}              # model_id -> host.CaptureBank over that model's assembler sources
        self.capture_staged = {}             # model_id -> [(assembler source, bytes)] until the next tick
        self.capture_fed = {}                # (model_id, assembler source) -> samples staged since the source was allocated
        self.capture_base = {}               # ... of them, those before the bank source's last reset: position 0 of its clock
        self.capture_waiting = {}            # model_id -> [(event, source name, label)] whose clips end behind what is written
        self.clip_reports = []               # the ticks' clips until take_clips()

    def allocate(self, source, model_id, capacity=None, source_rate=None):
        """The buffer of (source, model_id).  source_rate: the rate the source captures at; None or the model's effective rate
        = the bytes are written as they are, any other rate = resampled to the model's (see the class docstring)."""
        spec = self.orch.model_spec_for(model_id)
        if spec is None:
            raise OrchestratorError(f"unknown model: {model_id}")
        if source_rate is not None and source_rate <= 0:
            raise StreamError(f"invalid source sample rate: {source_rate}")
        model_rate = spec.effective_sample_rate()
        key = None if source_rate is None or source_rate == model_rate else (int(source_rate), int(model_rate))
        ab = self._allocate_buffer(source, model_id, spec, capacity)
        with self.mu:
            old = self.rates.pop((source, model_id), None)
            if old is not None:                                   # a re-allocated buffer starts a fresh resampler stream
                self._release_rate(source, old)
            if key is not None:
                self.rates[(source, model_id)] = key
                self._acquire_rate(source, key)
        return ab

    def _allocate_buffer(self, source, model_id, spec, capacity):
        clip, overlap, read = spec.buffer_dimensions()
        capacity = capacity if capacity is not None else 2 * clip
        if not self.native:
            ab = AnalysisBuffer(capacity, overlap, read, source)
            with self.mu:
                self.buffers[(source, model_id)] = ab
            return ab
        with self.mu:
            win = self.assemblers.get(model_id)
            if win is None or (win.overlap_size, win.read_size) != (overlap, read):
                if win is not None:                       # the model was re-registered with another geometry
                    for k in [k for k in self.buffers if k[1] == model_id]:
                        del self.buffers[k]
                        key = self.rates.pop(k, None)
                        if key is not None:
                            self._release_rate(k[0], key)
                    win.close()
                    for bank in (self.event_banks.pop(model_id, None), self.capture_banks.pop(model_id, None)):
                        if bank is not None:
                            bank.close()
                    for k in [k for k in self.capture_fed if k[0] == model_id]:
                        self._reset_capture(model_id, k[1], forget=True)
                win = self.assemblers[model_id] = NativeWindows(overlap, read, self.max_batch)
            old = self.buffers.pop((source, model_id), None)
            if old is not None:
                win.remove_source(old.index)
                self._reset_events(model_id, old.index)
            ab = self.buffers[(source, model_id)] = _NativeSource(win, win.add_source(source, capacity), source, model_id)
        return ab

    def remove(self, source, model_id=None):
        with self.mu:
            for k in [k for k in self.buffers if k[0] == source and (model_id is None or k[1] == model_id)]:
                ab = self.buffers.pop(k)
                if isinstance(ab, _NativeSource):
                    ab.win.remove_source(ab.index)
                    self._reset_events(k[1], ab.index)
                key = self.rates.pop(k, None)
                if key is not None:
                    self._release_rate(source, key)
        self.overruns.remove_source(source)

    def _reset_events(self, model_id, index):
        """(under self.mu) an assembler slot is reused by the next source: its pending detections go with the source."""
        bank = self.event_banks.get(model_id)
        if bank is not None and index < bank.max_sources:
            bank.reset(index)
        self.daylight.pop((model_id, index), None)
        self._reset_capture(model_id, index, forget=True)

    def _reset_capture(self, model_id, index, forget=False):
        """(under self.mu) the capture ring of an assembler slot starts again; forget: so does the slot's stream."""
        if self.capture is None:
            return
        bank = self.capture_banks.get(model_id)
        if bank is not None and index < bank.max_sources:
            bank.reset(index)
        key = (model_id, index)
        if forget:
            self.capture_fed.pop(key, None)
            self.capture_base.pop(key, None)
            self.capture_staged[model_id] = [it for it in self.capture_staged.get(model_id, []) if it[0] != index]
        else:
            self.capture_base[key] = self.capture_fed.get(key, 0)
        self.capture_waiting[model_id] = [it for it in self.capture_waiting.get(model_id, []) if int(it[0]["recording"]) != index]

    def _ring_write(self, ab, data):
        """One ring write; with capture the same bytes are staged for the model's capture bank."""
        ab.write(data)
        if self.capture is not None:
            with self.mu:
                self._stage_capture(ab, data)

    def _stage_capture(self, ab, data):
        """(under self.mu)"""
        if self.capture is None or not isinstance(ab, _NativeSource):
            return
        raw = _as_bytes(data).tobytes()
        self.capture_staged.setdefault(ab.model_id, []).append((ab.index, raw))
        key = (ab.model_id, ab.index)
        self.capture_fed[key] = self.capture_fed.get(key, 0) + len(raw) // (self.bit_depth // 8)

    def _capture_upload(self, model_id, spec):
        """The bytes staged since the last tick go up in one write call (the bank is made at the first)."""
        with self.mu:
            staged = self.capture_staged.pop(model_id, [])
            bank = self.capture_banks.get(model_id)
        staged = [it for it in staged if it[0] < self.capture.max_sources]
        if not staged:
            return
        try:
            if bank is None:
                bank = _host.CaptureBank(self.capture.max_sources, self.capture.seconds, spec.effective_sample_rate())
                with self.mu:
                    self.capture_banks[model_id] = bank
            bank.write(staged, self.bit_depth)
        except Exception as e:                                    # the frames are lost to the rings: their sources' clocks start again
            self.errors += len(staged)
            with self.mu:
                for index in {i for i, _ in staged}:
                    self._reset_capture(model_id, index)
            if self.on_error:
                self.on_error(model_id, sorted({f"source#{i}" for i, _ in staged}), e)

    def _capture_export(self, model_id, win, now):
        """The waiting events against the rings as they stand: those whose clips are complete are exported in one call."""
        with self.mu:
            waiting = self.capture_waiting.pop(model_id, [])
            bank = self.capture_banks.get(model_id)
            base = dict(self.capture_base)
        if not waiting or bank is None:
            return
        bps = self.bit_depth // 8
        hop, overlap = win.read_size // bps, win.overlap_size // bps
        settings = self.capture.export.settings(bank.rate)
        origins = np.full(bank.max_sources, -overlap, np.int64)   # the first window begins with `overlap` zeros
        for (m, index), n in base.items():
            if m == model_id and index < bank.max_sources:
                origins[index] -= n
        inside = [it for it in waiting if int(it[0]["recording"]) < bank.max_sources]
        ev = np.array([it[0] for it in inside], _host.EVENT) if inside else np.zeros(0, _host.EVENT)
        spans, status = bank.spans(ev, hop, settings, origins)
        room = max(1, min(self.capture.export.max_clips, 65535))
        ready = [i for i in range(len(inside)) if status[i] in (_host.CAPTURE_OK, _host.CAPTURE_CLAMPED)]
        later = [inside[i] for i in range(len(inside)) if status[i] == _host.CAPTURE_NOT_YET] + [inside[i] for i in ready[room:]]
        ready = ready[:room]
        clips = []
        if ready:
            try:
                clips = bank.export(spans[ready], settings)
            except Exception as e:
                self.errors += len(ready)
                if self.on_error:
                    self.on_error(model_id, sorted({inside[i][1] for i in ready}), e)
                ready = []
        reports = []
        made = {i: clips[j] for j, i in enumerate(ready[:len(clips)])}
        for i, (e, source, label) in enumerate(inside):
            if i not in made and status[i] != _host.CAPTURE_GONE:
                continue
            c = made.get(i)
            reports.append({"timestamp": now, "source": source, "model_id": model_id, "class_index": int(e["class_index"]), "label": label,
                            "first_window": int(e["first_window"]), "last_window": int(e["last_window"]), "status": int(status[i]),
                            "start": int(spans[i]["start"]), "length": int(spans[i]["length"]) if c is not None else 0,
                            "flac": c["flac"] if c is not None else None, "png": c["png"] if c is not None else None,
                            "loudness": c["loudness"] if c is not None else None})
        with self.mu:
            if later:
                self.capture_waiting[model_id] = later + self.capture_waiting.get(model_id, [])
            self.clip_reports.extend(reports)
        if reports and self.on_clips:
            self.on_clips(model_id, reports)

    def take_clips(self):
        """-> the detection clips since the last call, oldest first: {"timestamp", "source", "model_id", "class_index", "label",
        "first_window", "last_window", "status" (host.CAPTURE_OK, _CLAMPED: begun later than asked, or _GONE: no clip), "start" (the
        position of the clip's first sample on the source's capture clock), "length", "flac", "png", "loudness"}."""
        with self.mu:
            out, self.clip_reports = self.clip_reports, []
        return out

    def _event_bank(self, model_id, inst):
        """(under the model's inference lock) the bank of the model's assembler, created at the first tick with `events`."""
        bank = self.event_banks.get(model_id)
        if bank is None:
            n_classes = len(inst.labels)
            bank = _host.EventBank(n_classes, min(getattr(inst, "TOP_K", 10), n_classes), self.events, self.EVENT_SOURCES, extend=self.extend,
                                   dynamic=self.dynamic, guards=self.guards)
            with self.mu:
                self.event_banks[model_id] = bank
                for (mid, index), spans in self.daylight.items():
                    if mid == model_id and spans:
                        bank.set_daylight(index, spans)
        return bank

    def set_guards(self, guards):
        """New guards (a host.EventGuards) on every model's event bank from the next tick on; None turns them off."""
        if self.events is None or not self.native:
            raise StreamError("guards need events and the native rings")
        with self.mu:
            self.guards = guards
            for bank in self.event_banks.values():
                bank.set_guards(guards)

    def set_daylight(self, source, intervals, model_id=None):
        """The daylight intervals [(from_seconds, to_seconds), ...] of `source` (of its buffer for model_id, or for every model), in
        seconds of the source's audio clock - the audio written since it was allocated: at most host.EVENT_DAYLIGHT_SPANS, ascending
        and disjoint; [] for none.  Window w of the source begins at w * hop seconds (hop: the model's read size) and is in daylight
        when that instant lies in [from, to): both edges are rounded up to the next window start, from_window = ceil(from / hop) and
        to_window = ceil(to / hop).  The intervals are read when an event is flushed, so they have to cover the first windows of the
        events that are still pending - give the day's dawn and dusk ahead of time and replace them after the last event of the
        day has been answered.  Re-allocating or removing the source clears them."""
        if self.events is None or not self.native:
            raise StreamError("guards need events and the native rings")
        with self.mu:
            keys = [k for k, ab in self.buffers.items() if k[0] == source and (model_id is None or k[1] == model_id) and isinstance(ab, _NativeSource)]
            if not keys:
                raise StreamError(f"no native buffer of source {source!r}")
            for k in keys:
                spec = self.orch.model_spec_for(k[1])
                _, _, read = spec.buffer_dimensions()
                hop = read / (self.bit_depth // 8) / spec.effective_sample_rate()
                spans = [(max(0, int(math.ceil(lo / hop))), max(0, int(math.ceil(hi / hop)))) for lo, hi in intervals]
                spans = [sp for sp in spans if sp[1] > sp[0]]                     # (an interval that holds no window start)
                index = self.buffers[k].index
                self.daylight[(k[1], index)] = spans
                bank = self.event_banks.get(k[1])
                if bank is not None:
                    bank.set_daylight(index, spans)

    def take_events(self):
        """-> the detection events since the last call, oldest first: {"timestamp" (the batcher's clock at the tick), "source",
        "model_id", "class_index", "label", "first_window", "last_window", "best_window", "count", "confidence", "status"}; windows
        count the source's windows since it was allocated."""
        with self.mu:
            out, self.event_reports = self.event_reports, []
        return out

    def take_threshold_changes(self):
        """-> the threshold changes since the last call, oldest first: {"timestamp", "model_id", "class_index", "label",
        "previous_level", "new_level", "reason" (host.THRESHOLD_EXPIRY / THRESHOLD_HIGH_CONFIDENCE), "previous_value", "new_value",
        "confidence"}."""
        with self.mu:
            out, self.threshold_reports = self.threshold_reports, []
        return out

    # (under self.mu) one resampler stream per (source, rate pair) while a buffer of the source uses the pair
    def _acquire_rate(self, source, key):
        sk = (source,) + key
        if not self.native:
            if sk not in self.resamplers:
                self.resamplers[sk] = _host.StreamResampler(key[0], key[1])
            return
        if sk in self.bank_streams:
            return
        bank = self.banks.get(key)
        if bank is None:
            bank = self.banks[key] = _host.ResamplerBank(key[0], key[1], self.BANK_STREAMS)
        self.bank_streams[sk] = bank.add_stream()

    def _release_rate(self, source, key):
        if any(s == source and k == key for (s, _), k in self.rates.items()):
            return                                                # another model of the source still reads this pair
        sk = (source,) + key
        r = self.resamplers.pop(sk, None)
        if r is not None:
            r.close()
        st = self.bank_streams.pop(sk, None)
        if st is not None:
            self.banks[key].remove_stream(st)
            if key in self.pending:
                self.pending[key] = [it for it in self.pending[key] if it[1] != st]

    def set_processing(self, source, source_rate, filters=None, gain_db=0.0):
        """The source's EQ chain and input gain, as AddRoute gives them to the analysis consumer (audio_pipeline_service.go:
        1005-1006).  filters: conf.EqualizerSettings as a dict ({"enabled", "filters": [...]}) or a list of filter dicts
        (enabled), built for source_rate by host.build_filter_chain; gain_db: the source's gain (10^(dB/20)).  A new setting
        starts from zero filter state, as a freshly built chain does (see the class docstring)."""
        if source_rate is None or source_rate <= 0:
            raise StreamError(f"invalid source sample rate: {source_rate}")
        settings = {"enabled": True, "filters": list(filters)} if isinstance(filters, (list, tuple)) else filters
        chain = _host.build_filter_chain(settings, int(source_rate))
        gain = _host.gain_linear(gain_db)
        if chain is None and gain == 1.0:                         # the route's processing is skipped (router.go:848)
            self.clear_processing(source)
            return
        if self.eq_pending:                                       # frames captured under the old setting keep it
            self._drain_equalized()
        with self.mu:
            if self.eq_bank is None:
                self.eq_bank = _host.EqualizerBank(self.BANK_STREAMS)
            st = self.eq_streams.get(source)
            if st is None:
                st = self.eq_streams[source] = self.eq_bank.add_stream()
            self.eq_bank.set_chain(st, chain, gain)

    def clear_processing(self, source):
        """The source's frames go to its buffers as they are again."""
        if self.eq_pending:
            self._drain_equalized()
        with self.mu:
            st = self.eq_streams.pop(source, None)
            if st is not None:
                self.eq_bank.remove_stream(st)

    def set_sound_level(self, source, source_rate, interval_s=10, name=None):
        """The source's sound level monitor: a fresh Processor (NewProcessor(sid, sid, rate, interval)) reporting every interval_s
        seconds (below 1: 1); name defaults to the source.  Calling it again starts a fresh stream, as the reference builds a new
        Processor; frames queued before keep the old one."""
        if source_rate is None or source_rate <= 0:
            raise StreamError(f"invalid source sample rate: {source_rate}")
        rate = int(source_rate)
        self._drain_sound_levels_queued()
        with self.mu:
            old = self.sl_streams.pop(source, None)
            if old is not None:
                self.sl_banks[old[0]].remove_stream(old[1])
            bank = self.sl_banks.get(rate)
            if bank is None:
                bank = self.sl_banks[rate] = _host.SoundLevelBank(rate, self.BANK_STREAMS)
            self.sl_streams[source] = (rate, bank.add_stream(interval_s), source if name is None else name)

    def clear_sound_level(self, source):
        """The source's monitor stops; frames queued before still count."""
        self._drain_sound_levels_queued()
        with self.mu:
            old = self.sl_streams.pop(source, None)
            if old is not None:
                self.sl_banks[old[0]].remove_stream(old[1])

    def set_audio_level(self, source, name=None):
        """The source's input level meter; name defaults to the source.  Calling it again starts a fresh stream (empty
        accumulators); frames queued before keep the old one."""
        if self.al_pending:
            self._drain_audio_levels()
        with self.mu:
            if self.al_bank is None:
                self.al_bank = _host.LevelBank(self.BANK_STREAMS)
            old = self.al_streams.pop(source, None)
            if old is not None:
                self.al_bank.remove_stream(old[0])
            self.al_streams[source] = (self.al_bank.add_stream(), source if name is None else name)

    def clear_audio_level(self, source):
        """The source's meter stops; frames queued before still count."""
        if self.al_pending:
            self._drain_audio_levels()
        with self.mu:
            old = self.al_streams.pop(source, None)
            if old is not None:
                self.al_bank.remove_stream(old[0])

    def take_audio_levels(self):
        """-> the measurements since the last call, oldest first: {"timestamp" (the batcher's clock when the measurement came
        back), "source", "name", "level" (0..100), "clipping" (bool)}, one per frame written to a metered source."""
        with self.mu:
            out, self.al_reports = self.al_reports, []
        return out

    def audio_level_stats(self, source, reset=False):
        """host.LevelBank.stats of the source's stream: what the reference's five-minute summary logs (reset: and starts again)."""
        if self.al_pending:
            self._drain_audio_levels()
        with self.mu:
            if source not in self.al_streams:
                raise StreamError(f"source {source!r} has no audio level meter")
            return self.al_bank.stats(self.al_streams[source][0], reset)

    def _audio_level_call(self, items):
        """(under self.mu) One bank call over items [(source, stream, pcm bytes), ...] -> self.al_reports, or the error."""
        try:
            recs = self.al_bank.process([(st, raw) for _, st, raw in items])
        except Exception as e:
            self.errors += len(items)
            return e
        for (src, _, _), r in zip(items, recs):
            name = self.al_streams.get(src, (None, src))[1]
            self.al_reports.append({"timestamp": self.clock(), "source": src, "name": name, "level": int(r["level"]),
                                    "clipping": bool(r["clipping"])})
        return None

    def _measure_level(self, source, stream, data):
        """write()'s frame of a metered source: queued (native) or measured at once (python)."""
        raw = _as_bytes(data).tobytes()
        with self.mu:
            if self.native:
                self.al_pending.append((source, stream, raw))
                return
            err = self._audio_level_call([(source, stream, raw)])
        if err is not None and self.on_error:
            self.on_error(None, [source], err)

    def _drain_audio_levels(self):
        """Native: every metered source's queued frames through one device call (host.LevelBank)."""
        with self.mu:
            items, self.al_pending = self.al_pending, []
            err = self._audio_level_call(items) if items else None
        if err is not None and self.on_error:
            self.on_error(None, sorted({src for src, *_ in items}), err)

    def take_sound_levels(self):
        """-> the finished reports since the last call, oldest first: {"timestamp" (the batcher's clock when the report was
        made), "source", "name", "duration_seconds", "octave_bands": {key: {"center_frequency_hz", "min_db", "max_db", "mean_db",
        "sample_count"}}}."""
        with self.mu:
            out, self.sl_reports = self.sl_reports, []
        return out

    def _drain_sound_levels_queued(self):
        if self.eq_pending:                                       # a monitored source's processed frames are queued behind them
            self._drain_equalized()
        if self.sl_pending:
            self._drain_sound_levels()

    def _sound_level_reports(self, items, reports):
        """(under self.mu) bank reports of the call over items [(source, stream, pcm bytes), ...] -> self.sl_reports."""
        for r in reports:
            src = items[r["frame"]][0]
            name = self.sl_streams.get(src, (None, None, src))[2]
            self.sl_reports.append({"timestamp": self.clock(), "source": src, "name": name, "duration_seconds": r["duration_seconds"],
                                    "octave_bands": r["octave_bands"]})

    def _drain_sound_levels(self):
        """Native: every monitored source's queued frames through one device call per source rate (host.SoundLevelBank)."""
        failed = []
        with self.mu:
            pending, self.sl_pending = self.sl_pending, {}
            for rate, items in pending.items():
                try:
                    reports = self.sl_banks[rate].process([(st, raw) for _, st, raw in items])
                except Exception as e:
                    self.errors += len(items)
                    failed.append((sorted({src for src, *_ in items}), e))
                    continue
                self._sound_level_reports(items, reports)
        for sources, e in failed:
            if self.on_error:
                self.on_error(None, sources, e)

    def write(self, source, data):
        """Capture side: the same bytes go to every model's buffer of that source; a buffer of another rate gets them resampled
        (once per rate pair: buffer_consumer.go:184-210).  A processed source's bytes are processed first (set_processing)."""
        with self.mu:
            st = self.eq_streams.get(source)
            al = self.al_streams.get(source)
        if al is not None:                                        # the level route: the frame as given, before the EQ
            self._measure_level(source, al[0], data)
        if st is not None:
            raw = _as_bytes(data).tobytes()
            try:
                if len(raw) % BYTES_PER_SAMPLE:
                    raise StreamError(f"frame of {len(raw)} bytes is not whole 16-bit samples")
                if self.native:
                    with self.mu:
                        self.eq_pending.append((source, st, raw))
                    return
                data = self.eq_bank.process([(st, raw)])[0]
            except Exception as e:                                # router.go:1064-1073: the frame is dropped, the route goes on
                self.errors += 1
                if self.on_error:
                    self.on_error(None, [source], e)
                return
        self._fan_out(source, data)

    def _fan_out(self, source, data):
        sl = None
        with self.mu:
            mon = self.sl_streams.get(source)
            raw_sl = _as_bytes(data).tobytes() if mon is not None else b""
            raw_sl = raw_sl[:len(raw_sl) & ~1]                    # whole samples (sound_level_consumer.go:109-111)
            if raw_sl:                                            # an empty frame is not a call (:117)
                sl = (source, mon[1], raw_sl)
                if self.native:
                    self.sl_pending.setdefault(mon[0], []).append(sl)
                    sl = None
                else:
                    bank = self.sl_banks[mon[0]]
            groups = {}
            for (s, m), ab in self.buffers.items():
                if s == source:
                    groups.setdefault(self.rates.get((s, m)), []).append(ab)
            abs_ = groups.pop(None, [])
            resampled = []
            if groups:
                raw = _as_bytes(data).tobytes()
                for key, targets in groups.items():
                    if self.native:
                        self.pending.setdefault(key, []).append((source, self.bank_streams[(source,) + key], raw, targets))
                    else:
                        resampled.append((self.resamplers[(source,) + key], targets))
        for ab in abs_:
            self._ring_write(ab, data)
        for r, targets in resampled:
            out = r.resample_into(raw)
            for ab in targets:
                self._ring_write(ab, out)
        if sl is not None:                                        # python: one monitor call per write
            with self.mu:
                try:
                    self._sound_level_reports([sl], bank.process([sl[1:]]))
                except Exception as e:
                    self.errors += 1
                    err = e
                else:
                    err = None
            if err is not None and self.on_error:
                self.on_error(None, [source], err)

    def _bank_call(self, bank, items, failed):
        """(under self.mu) One call of `bank` (host.EqualizerBank / host.ResamplerBank) for the queued [(source, stream, pcm bytes,
        buffers), ...], `buffers` being the rings an item may be written to directly.  When every item has exactly one and all of
        them are in one assembler the results go straight into its rings (bank.write_windows) -> None; otherwise they come back,
        one bytes object per item.  A failed call loses the frames of its items (on_error, as the reference logs a failed
        applyProcessing or resample and goes on): they count in self.errors, (sources, error) goes to `failed` -> None."""
        try:
            wins = {id(ab.win) for *_, bufs in items for ab in bufs}
            if self.capture is None and len(wins) == 1 and all(len(bufs) == 1 for *_, bufs in items):   # (capture stages what the rings get)
                bank.write_windows(items[0][3][0].win, [(st, bufs[0].index, raw) for _, st, raw, bufs in items])
                return None
            return bank.process([(st, raw) for _, st, raw, _ in items])
        except Exception as e:
            self.errors += len(items)
            failed.append((sorted({src for src, *_ in items}), e))
            return None

    def _drain_equalized(self):
        """Native: every processed source's queued frames through one device call (host.EqualizerBank), then on to the source's
        buffers: straight into the rings when each frame's source has one buffer, at its model's rate, and all of them are in one
        assembler; otherwise the results come back and take write()'s path, so they also reach this tick's resampler queue."""
        failed = []
        with self.mu:
            pending, self.eq_pending = self.eq_pending, []
            if not pending:
                return
            bufs, resampled = {}, {s for s, _ in self.rates}
            for (s, _), ab in self.buffers.items():
                bufs.setdefault(s, []).append(ab)
            # a monitored source's processed frames come back (its monitor is queued from them in _fan_out)
            items = [(src, st, raw, [] if src in resampled or src in self.sl_streams else bufs.get(src, [])) for src, st, raw in pending]
            outs = self._bank_call(self.eq_bank, items, failed)
        for sources, e in failed:
            if self.on_error:
                self.on_error(None, sources, e)
        for (src, *_), out in zip(items, outs or []):
            self._fan_out(src, out)

    def _drain_resampled(self):
        """Native: every rate pair's queued frames through one device call (host.ResamplerBank), one ring write per frame: straight
        into the rings when each frame has one buffer and all of them are in one assembler; otherwise the results come back and
        are written to every buffer of the frame's group."""
        failed = []
        with self.mu:
            pending, self.pending = self.pending, {}
            live = {id(ab) for ab in self.buffers.values()}
            for key, items in pending.items():
                items = [(src, st, raw, [ab for ab in targets if id(ab) in live]) for src, st, raw, targets in items]
                outs = self._bank_call(self.banks[key], items, failed)
                for (*_, targets), out in zip(items, outs or []):
                    for ab in targets:
                        ab.write(out)
                        self._stage_capture(ab, out)
        for sources, e in failed:
            if self.on_error:
                self.on_error(None, sources, e)

    def _tick_native(self):
        with self.mu:
            wins = list(self.assemblers.items())
            names = {(id(ab.win), ab.index): src for (src, _), ab in self.buffers.items() if isinstance(ab, _NativeSource)}
        sent = 0
        def name(win, i):
            return None if i < 0 else names.get((id(win), i), f"source#{i}")

        tick_events = []

        def one_tick(inst, win, model_id=None):
            # an instance that can run the whole tick in the library does (rows assembled under the device's work on the
            # previous chunk); anything else gets the collected rows
            if self.events is not None and hasattr(inst, "predict_windows"):
                bank = self._event_bank(model_id, inst)
                if self.dynamic is not None:
                    self.bank_now = max(self.bank_now, int(round((self.clock() - self.created) * 1000.0)))
                    bank.set_now(self.bank_now)
                if hasattr(inst, "predict_windows_events"):       # rows and events in one call
                    idxs, rows, lists, ev = inst.predict_windows_events(win, bank, self.bit_depth)
                else:                                             # the bank is fed the rows the tick returned
                    idxs, rows, lists = inst.predict_windows(win, self.bit_depth)
                    number = {label: i for i, label in enumerate(inst.labels)}
                    conf = np.full((len(idxs), bank.k), np.nan, np.float32)
                    idx = np.full((len(idxs), bank.k), -1, np.int32)
                    for r, lst in enumerate(lists):
                        for j, (label, c) in enumerate(lst[:bank.k]):
                            conf[r, j], idx[r, j] = c, number[label]
                    ev = bank.process(idxs, conf, idx)
                tick_events.append((inst, ev))
                return idxs, rows, lists
            if hasattr(inst, "predict_windows"):
                return inst.predict_windows(win, self.bit_depth)
            idxs, rows = win.collect(self.max_batch)
            try:
                return idxs, rows, (_pcm_windows_predict(inst, rows, self.bit_depth) if idxs else [])
            except Exception as e:
                e.sources = idxs                              # (consumed all the same)
                raise

        for model_id, win in wins:
            if self.capture is not None and self.orch.model_spec_for(model_id) is not None:
                self._capture_upload(model_id, self.orch.model_spec_for(model_id))
            while True:
                spec = self.orch.model_spec_for(model_id)
                if spec is None or not self.orch.is_model_active(model_id):   # consumed, not analysed (buffer_manager.go:478-481)
                    idxs, _ = win.collect(self.max_batch)
                    if len(idxs) < min(self.max_batch, win.max_batch):
                        break
                    continue
                if not win.ready():                               # nothing to do: no inference lock, no invoke counted
                    break
                now = self.clock()
                start = now - (self.pre_capture_s + spec.clip_length_s)
                t0 = time.perf_counter()
                try:
                    idxs, rows, lists = self.orch.predict_model(model_id, lambda inst: one_tick(inst, win, model_id))
                except Exception as e:
                    lost = [name(win, i) for i in getattr(e, "sources", [])]
                    self.errors += max(1, len(lost))
                    if self.on_error:
                        self.on_error(model_id, lost, e)
                    break
                if not idxs:
                    break
                for inst, ev in tick_events:
                    reports = [{"timestamp": now, "source": name(win, int(e["recording"])), "model_id": model_id, "class_index": int(e["class_index"]),
                                "label": inst.labels[int(e["class_index"])], "first_window": int(e["first_window"]),
                                "last_window": int(e["last_window"]), "best_window": int(e["best_window"]), "count": int(e["count"]),
                                "confidence": float(e["confidence"]), "status": int(e["status"])} for e in ev]
                    if reports:
                        with self.mu:
                            self.event_reports.extend(reports)
                            if self.capture is not None:
                                self.capture_waiting.setdefault(model_id, []).extend(
                                    (e.copy(), r["source"], r["label"]) for e, r in zip(ev, reports) if int(e["status"]) == 0)
                        if self.on_events:
                            self.on_events(model_id, reports)
                    if self.dynamic is not None:
                        changes = [{"timestamp": now, "model_id": model_id, "class_index": int(c["class_index"]),
                                    "label": inst.labels[int(c["class_index"])], "previous_level": int(c["previous_level"]),
                                    "new_level": int(c["new_level"]), "reason": int(c["reason"]), "previous_value": float(c["previous_value"]),
                                    "new_value": float(c["new_value"]), "confidence": float(c["confidence"])}
                                   for c in self.event_banks[model_id].threshold_changes()]
                        if changes:
                            with self.mu:
                                self.threshold_reports.extend(changes)
                            if self.on_threshold_changes:
                                self.on_threshold_changes(model_id, changes)
                del tick_events[:]
                sources = [name(win, i) for i in idxs]
                sent += _emit_results(self.orch, rows, lists, time.perf_counter() - t0, [start] * len(idxs), [now] * len(idxs), sources,
                                      model_id, self.queue, self.overruns)
                if len(idxs) < min(self.max_batch, win.max_batch):
                    break
            if self.capture is not None:
                self._capture_export(model_id, win, self.clock())
        return sent

    def close(self):
        with self.mu:
            for win in self.assemblers.values():
                win.close()
            self.assemblers.clear()
            self.buffers.clear()
            for r in list(self.resamplers.values()) + list(self.banks.values()):
                r.close()
            self.resamplers.clear()
            self.banks.clear()
            self.bank_streams.clear()
            self.pending.clear()
            self.rates.clear()
            if self.eq_bank is not None:
                self.eq_bank.close()
            self.eq_bank = None
            self.eq_streams.clear()
            self.eq_pending.clear()
            for bank in self.sl_banks.values():
                bank.close()
            self.sl_banks.clear()
            if self.al_bank is not None:
                self.al_bank.close()
            self.al_bank = None
            self.al_streams.clear()
            self.al_pending.clear()
            for bank in list(self.event_banks.values()) + list(self.capture_banks.values()):
                bank.close()
            self.event_banks.clear()
            self.capture_banks.clear()
            for d in (self.capture_staged, self.capture_fed, self.capture_base, self.capture_waiting):
                d.clear()
            self.sl_streams.clear()
            self.sl_pending.clear()

    def tick(self):
        if self.native:
            if self.al_pending:
                self._drain_audio_levels()
            if self.eq_pending:
                self._drain_equalized()
            if self.sl_pending:
                self._drain_sound_levels()
            if self.pending:
                self._drain_resampled()
            return self._tick_native()
        with self.mu:
            items = list(self.buffers.items())
        per_model = {}
        for (source, model_id), ab in items:
            win = ab.read()
            if win is None:
                continue
            spec = self.orch.model_spec_for(model_id)
            if spec is None or not self.orch.is_model_active(model_id):       # (unloaded since the last tick: consumed, not analysed)
                continue
            now = self.clock()
            start = now - (self.pre_capture_s + spec.clip_length_s)       # beginTimeOffset, buffer_manager.go:490-491
            per_model.setdefault(model_id, []).append((source, win, start, now))
        sent = 0
        for model_id, ws in per_model.items():
            for lo in range(0, len(ws), self.max_batch):
                part = ws[lo:lo + self.max_batch]
                try:
                    sent += process_windows(self.orch, np.stack([w for _, w, _, _ in part]), [s for _, _, s, _ in part],
                                            [c for _, _, _, c in part], [src for src, _, _, _ in part], model_id, self.queue,
                                            self.overruns, self.bit_depth)
                except Exception as e:                    # buffer_manager.go:494-499: the monitor logs the error and keeps polling
                    self.errors += len(part)
                    if self.on_error:
                        self.on_error(model_id, [src for src, _, _, _ in part], e)
        return sent
