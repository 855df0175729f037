"""Dynamic thresholds (include/bnhip.h, "Detection events: dynamic thresholds"), restated in plain Python as a wrapper around a
streaming restatement of the bank (evbankref.EventBank, or evxref.EventBank for a bank created extended): the per-class learning
state, shared by all sources, and the five steps of a process or flush call.  A dynamic device bank (host.EventBank(dynamic=)) is
pinned to this class in tests/test_event_dynamic.py, and this class to a literal table of the reference's cases in
tests/test_event_dynamic_ref.py.

The dynamic is any object with class_dynamic (or None: every class learns), trigger, min_threshold, valid and cooldown; None:
learning is off.  Confidences and thresholds are float32, the product base * mult and the clamp are float64, times are Python ints."""
import numpy as np

from evref import KEPT

EXPIRY, HIGH_CONFIDENCE = 0, 1
INT32_MAX = 2 ** 31 - 1
CHANGE = np.dtype([("class_index", "<i4"), ("previous_level", "<i4"), ("new_level", "<i4"), ("reason", "<i4"), ("previous_value", "<f4"),
                   ("new_value", "<f4"), ("confidence", "<f4"), ("pad", "<i4")])
MULT = (1.0, 0.75, 0.5, 0.25)


def threshold(base, level, min_threshold):
    """Step 2 for one class: level 0 answers base bit for bit; a NaN base stays NaN."""
    base = np.float32(base)
    if level <= 0:
        return base
    v, lo = np.float64(base) * np.float64(MULT[level]), np.float64(np.float32(min_threshold))
    return np.float32(lo if v < lo else v)


class DynamicBank:
    def __init__(self, inner, dyn):
        self.inner, self.n_classes = inner, inner.n_classes
        self.base = inner.thr.copy()
        n = self.n_classes
        self.level, self.count = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.expires, self.learned_at = np.zeros(n, np.int64), np.full(n, -1, np.int64)
        self.now, self.changes = 0, np.zeros(0, CHANGE)
        self.trigger, self.min_threshold, self.valid, self.cooldown = np.float32(0), np.float32(0), 1, 0
        self.set_dynamic(dyn)

    # ---- settings
    def set_dynamic(self, dyn):
        self.dyn = dyn
        if dyn is None:
            self.dynamic = np.zeros(self.n_classes, bool)
            return
        self.dynamic = np.ones(self.n_classes, bool) if dyn.class_dynamic is None else np.array(dyn.class_dynamic, np.uint8) != 0
        self.trigger, self.min_threshold = np.float32(dyn.trigger), np.float32(dyn.min_threshold)
        self.valid, self.cooldown = int(dyn.valid), int(dyn.cooldown)

    def set_filter(self, flt):
        self.inner.set_filter(flt)
        self.base = self.inner.thr.copy()

    def set_extend(self, ext):
        self.inner.set_extend(ext)

    def set_now(self, now):
        if not 0 <= now < 2 ** 62 or now < self.now:
            raise ValueError("bank time never decreases")
        self.now = int(now)

    # ---- the state's surface
    def thresholds(self):
        """-> level, high_count, expires, learned_at, current"""
        cur = np.array([threshold(self.base[c], int(self.level[c]), self.min_threshold) if self.dynamic[c] else self.base[c]
                        for c in range(self.n_classes)], np.float32)
        return self.level.copy(), self.count.copy(), self.expires.copy(), self.learned_at.copy(), cur

    def restore_thresholds(self, level, high_count, expires, learned_at):
        level, high_count = np.asarray(level, np.int32), np.asarray(high_count, np.int32)
        expires, learned_at = np.asarray(expires, np.int64), np.asarray(learned_at, np.int64)
        ok = (level >= 0) & (level <= 3) & (high_count >= 0) & (level == np.minimum(high_count, 3)) & (learned_at >= -1) & (expires >= 0)
        if not ok.all():
            raise ValueError("not a threshold state")
        self.level, self.count, self.expires, self.learned_at = level.copy(), high_count.copy(), expires.copy(), learned_at.copy()

    def reset_thresholds(self, c=-1):
        which = slice(None) if c < 0 else c
        self.level[which], self.count[which], self.expires[which], self.learned_at[which] = 0, 0, 0, -1

    def take_changes(self):
        return self.changes

    # ---- the calls
    def _call(self, run, rows):
        """run(): the inner bank's call under inner.thr -> its events; rows: the call's counted (conf [k], idx [k]) rows."""
        if self.dyn is None:
            self.inner.thr = self.base.copy()
            out = run()
            self.changes = np.zeros(0, CHANGE)
            return out
        now, dynamic, base = self.now, self.dynamic, self.base
        L, n, E, A = self.level.copy(), self.count.copy(), self.expires.copy(), self.learned_at.copy()
        records = []
        # 1 expiry
        for c in np.flatnonzero(dynamic & (n > 0) & (now > E)):
            if L[c] != 0:
                records.append((int(c), int(L[c]), 0, EXPIRY, threshold(base[c], int(L[c]), self.min_threshold), base[c], np.float32(0), 0))
            L[c], n[c], A[c] = 0, 0, -1
        # 2 the call's thresholds
        thr = base.copy()
        for c in np.flatnonzero(dynamic & (L > 0)):
            thr[c] = threshold(base[c], int(L[c]), self.min_threshold)
        # 3 the bank's rule (a refusal leaves here: nothing has changed)
        self.inner.thr = thr
        out = run()
        # 4 touch
        for conf, idx in rows:
            for x, c in zip(conf, idx.tolist()):
                if c < 0 or c >= self.n_classes or self.inner.vetoed[c] or not dynamic[c] or n[c] <= 0:
                    continue
                if x > thr[c] and x > base[c]:
                    E[c] = now + self.valid
        # 5 learn
        best = {}
        for e in out:
            c, x = int(e["class_index"]), np.float32(e["confidence"])
            if int(e["status"]) == KEPT and dynamic[c] and x > self.trigger and x >= base[c]:
                best[c] = max(best.get(c, x), x)
        for c, x in best.items():
            E[c] = now + self.valid
            if A[c] < 0 or now - int(A[c]) >= self.cooldown:
                n[c], A[c] = min(int(n[c]) + 1, INT32_MAX), now
                l2 = min(int(n[c]), 3)
                if l2 != L[c]:
                    records.append((c, int(L[c]), l2, HIGH_CONFIDENCE, threshold(base[c], int(L[c]), self.min_threshold),
                                    threshold(base[c], l2, self.min_threshold), x, 0))
                L[c] = l2
        records.sort(key=lambda r: (r[0], r[3]))
        self.level, self.count, self.expires, self.learned_at = L, n, E, A
        self.changes = np.array(records, CHANGE) if records else np.zeros(0, CHANGE)
        return out

    def process(self, sources, conf, idx, cap=None):
        k = self.inner.k
        conf = np.asarray(conf, np.float32).reshape(len(sources), k)
        idx = np.asarray(idx, np.int32).reshape(len(sources), k)
        rows = [(conf[r], idx[r]) for r, s in enumerate(sources) if int(s) >= 0]
        return self._call(lambda: self.inner.process(sources, conf, idx, cap), rows)

    def flush(self, source=-1, cap=None):
        return self._call(lambda: self.inner.flush(source, cap), [])

    def pending(self, cap=None):
        return self.inner.pending(cap)

    def reset(self, source=-1):
        self.inner.reset(source)

    def clock(self, source):
        return self.inner.clock(source)
