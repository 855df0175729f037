"""Extended capture's sliding deadline (include/bnhip.h, "Detection events: extended capture"), restated in plain Python in two
parts: the one-shot rule over sorted rows (`events`), to which bnhip_detection_events_extended and the extended analysis entries are
pinned, and the streaming rule with a deadline per live event (`EventBank`), to which an extended device bank is pinned.  The two are
pinned to each other, and to evref.events where no class slides, in tests/test_event_extend_ref.py.

The filter is what evref takes.  The extend is any object with class_extended (or None: every class slides), max_windows, short_wait,
medium_from, medium_wait, long_from and long_wait, in windows; None: no class slides."""
import numpy as np

import evbankref
from evbankref import TooSmall                                                  # noqa: F401 (the callers' name for it)
from evref import EVENT, FEW, KEEP_DROPPED, KEPT, VETOED, marks

PENDING = evbankref.PENDING


def deadline(b, w, hold, ext):
    """The deadline that a hit at window w gives an event of a sliding class opened at window b."""
    t = w - b
    wait = max(hold, ext.short_wait) if t < ext.medium_from else ext.medium_wait if t < ext.long_from else ext.long_wait
    return min(w + wait, b + ext.max_windows)


def slides(ext, c):
    return ext is not None and (ext.class_extended is None or bool(ext.class_extended[c]))


def longest_wait(hold, ext):
    return hold if ext is None else max(hold, ext.short_wait, ext.medium_wait, ext.long_wait)


def events(rows, flt, ext):
    """-> the events (EVENT), ascending by (recording, class_index, first_window)."""
    hold, min_count = int(flt.hold_windows), int(flt.min_count)
    hits, vetoed = marks(rows, flt)
    out = []
    for r, c in sorted(hits):
        group = sorted(hits[(r, c)], key=lambda h: h[0])                # stable: equal windows stay in row order
        sl = slides(ext, c)
        found = []
        for w, x in group:
            if not found or w >= found[-1]["d"]:
                found.append({"b": w, "last": w, "count": 1, "conf": x, "best": w, "d": deadline(w, w, hold, ext) if sl else w + hold})
                continue
            e = found[-1]
            e["last"], e["count"] = w, e["count"] + 1
            if x > e["conf"]:                                            # a tie keeps the earliest
                e["conf"], e["best"] = x, w
            if sl:
                e["d"] = deadline(e["b"], w, hold, ext)                  # the last hit's deadline stands
        for e in found:
            if e["count"] < min_count:
                status = FEW
            elif any(e["b"] <= v < e["d"] for v in vetoed.get(r, ())):
                status = VETOED
            else:
                status = KEPT
            if status == KEPT or (int(flt.flags) & KEEP_DROPPED):
                out.append((r, c, e["b"], e["last"], e["best"], e["count"], e["conf"], status))
    return np.array(out, EVENT) if out else np.zeros(0, EVENT)


class EventBank(evbankref.EventBank):
    """evbankref.EventBank created extended: a live event is [first, last, best, count, conf, deadline]; flush, pending, reset and
    set_filter are the base's."""

    def __init__(self, max_sources, n_classes, k, flt, ext):
        super().__init__(max_sources, n_classes, k, flt)
        self.longest_wait = longest_wait(self.hold, ext)
        self.slots_per_source = min(self.k * self.longest_wait, self.n_classes)
        self.set_extend(ext)

    def set_extend(self, ext):
        if longest_wait(self.hold, ext) > self.longest_wait:
            raise ValueError("the longest wait is fixed for the bank's life")
        self.ext = ext

    def process(self, sources, conf, idx, cap=None):
        conf = np.asarray(conf, np.float32).reshape(len(sources), self.k)
        idx = np.asarray(idx, np.int32).reshape(len(sources), self.k)
        work, out = {}, []
        for r, s in enumerate(sources):
            s = int(s)
            if s < 0:
                continue
            if s not in work:
                work[s] = self.src[s].copy() if s in self.src else evbankref._Source()
            S, w = work[s], work[s].clock
            for x, c in zip(conf[r], idx[r].tolist()):
                if c < 0 or c >= self.n_classes:
                    continue
                if self.vetoed[c]:
                    if x > self.veto_thr:
                        S.veto = w
                elif x > self.thr[c]:
                    sl = slides(self.ext, c)
                    e = S.live.get(c)
                    if e is None:
                        S.live[c] = [w, w, w, 1, x, deadline(w, w, self.hold, self.ext) if sl else w + self.hold]
                    else:
                        e[1], e[3] = w, e[3] + 1
                        if x > e[4]:
                            e[4], e[2] = x, w
                        if sl:
                            e[5] = deadline(e[0], w, self.hold, self.ext)
            for c in [c for c, e in S.live.items() if e[5] <= w + 1]:
                e = S.live.pop(c)
                out.append((s, c, e[0], e[1], e[2], e[3], e[4], self._status(S, e)))
            S.clock = w + 1
        out = self._answer(out, cap)
        self.src.update(work)
        return out
