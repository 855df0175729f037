"""The detection-event rule in streaming form (include/bnhip.h, "Detection events: the real-time bank"), restated in plain Python:
a clock and a dict of live events per source.  The device bank (bnhip_event_bank_*, host.EventBank) is pinned to this class, and this
class to the one-shot rule (evref.events) in tests/test_event_bank_ref.py.

A row is one window's top-k: k results (conf, idx), idx < 0 no result.  The filter is any object with class_threshold, class_veto (or
None), veto_threshold, hold_windows, min_count and flags."""
import numpy as np

from evref import EVENT, FEW, KEEP_DROPPED, KEPT, VETOED

PENDING = -1


class TooSmall(Exception):
    """A call that answers more events than `cap`: `.needed` of them; nothing has changed."""

    def __init__(self, needed):
        super().__init__(f"the call answers {needed} events")
        self.needed = needed


class _Source:
    def __init__(self):
        self.clock, self.live, self.veto = 0, {}, -1      # live: class -> [first, last, best, count, conf]

    def copy(self):
        c = _Source()
        c.clock, c.live, c.veto = self.clock, {k: list(v) for k, v in self.live.items()}, self.veto
        return c


class EventBank:
    def __init__(self, max_sources, n_classes, k, flt):
        self.max_sources, self.n_classes, self.k, self.hold = int(max_sources), int(n_classes), int(k), int(flt.hold_windows)
        self.slots_per_source = min(self.k * self.hold, self.n_classes)
        self.src = {}
        self.set_filter(flt)

    def set_filter(self, flt):
        if int(flt.hold_windows) != self.hold:
            raise ValueError("hold_windows is fixed for the bank's life")
        self.thr = np.array(flt.class_threshold, np.float32)
        self.vetoed = np.zeros(self.n_classes, np.uint8) if flt.class_veto is None else np.array(flt.class_veto, np.uint8)
        self.veto_thr, self.min_count, self.flags = np.float32(flt.veto_threshold), int(flt.min_count), int(flt.flags)

    def clock(self, source):
        return self.src[source].clock if source in self.src else 0

    def _status(self, S, e):
        if e[3] < self.min_count:
            return FEW
        return VETOED if S.veto >= e[0] else KEPT

    def _answer(self, out, cap):
        out = [e for e in out if e[-1] in (KEPT, PENDING) or (self.flags & KEEP_DROPPED)]
        if cap is not None and len(out) > cap:
            raise TooSmall(len(out))
        out.sort(key=lambda e: e[:3])
        return np.array(out, EVENT) if out else np.zeros(0, EVENT)

    def process(self, sources, conf, idx, cap=None):
        """rows r of sources[r] (< 0: skipped), conf / idx [n_rows, k] -> the events that became due (EVENT)."""
        conf = np.asarray(conf, np.float32).reshape(len(sources), self.k)
        idx = np.asarray(idx, np.int32).reshape(len(sources), self.k)
        work, out = {}, []
        for r, s in enumerate(sources):
            s = int(s)
            if s < 0:
                continue
            if s not in work:
                work[s] = self.src[s].copy() if s in self.src else _Source()
            S, w = work[s], work[s].clock
            for x, c in zip(conf[r], idx[r].tolist()):
                if c < 0 or c >= self.n_classes:
                    continue
                if self.vetoed[c]:
                    if x > self.veto_thr:                                # float32, strict; false for a NaN on either side
                        S.veto = w
                elif x > self.thr[c]:
                    e = S.live.get(c)
                    if e is None:
                        S.live[c] = [w, w, w, 1, x]
                    else:
                        e[1], e[3] = w, e[3] + 1
                        if x > e[4]:                                     # a tie keeps the earliest
                            e[4], e[2] = x, w
            for c in [c for c, e in S.live.items() if e[0] + self.hold <= w + 1]:
                e = S.live.pop(c)
                out.append((s, c, e[0], e[1], e[2], e[3], e[4], self._status(S, e)))
            S.clock = w + 1
        out = self._answer(out, cap)
        self.src.update(work)                                            # the commit: nothing changed before here
        return out

    def flush(self, source=-1, cap=None):
        which = sorted(self.src) if source < 0 else [source] if source in self.src else []
        out = [(s, c, e[0], e[1], e[2], e[3], e[4], self._status(self.src[s], e)) for s in which for c, e in self.src[s].live.items()]
        out = self._answer(out, cap)
        for s in which:
            self.src[s].live = {}
        return out

    def pending(self, cap=None):
        return self._answer([(s, c, e[0], e[1], e[2], e[3], e[4], PENDING) for s in self.src for c, e in self.src[s].live.items()], cap)

    def reset(self, source=-1):
        if source < 0:
            self.src = {}
        else:
            self.src.pop(source, None)
