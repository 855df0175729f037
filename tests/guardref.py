"""The dog-bark and daylight filters (include/bnhip.h, "Detection events: dog-bark and daylight filters"), restated in plain Python
in two parts: the one-shot rule over sorted rows (`events`, built on evxref.events), to which bnhip_detection_events_guarded and the
guarded analysis entries are pinned, and the streaming rule (`EventBank`, an evxref.EventBank with a dog window per source and
daylight spans per source), to which a device bank under guards is pinned.  The two are pinned to each other, and to evxref where
the guards do nothing, in tests/test_event_guards_ref.py.  Integer and float32 compares only.

The filter and the extend are what evxref takes.  The guards are any object with class_dog, class_dog_filtered, class_daylight (each
a table or None), dog_threshold, dog_remember_windows and - the one-shot rule only - daylight_spans (rows (recording, from, to), or
None); None: no guards."""
import types

import numpy as np

import evbankref
import evxref
from evref import EVENT, FEW, KEEP_DROPPED, KEPT, VETOED                        # noqa: F401 (the callers' names for them)
from evxref import PENDING, TooSmall, deadline, slides                          # noqa: F401

DOG, DAYLIGHT = 3, 4
DAYLIGHT_SPANS = 8


def _table(t, c):
    return t is not None and bool(t[c])


def dog_hit(guards, c, x):
    """float32, strict; false for a NaN on either side."""
    return guards is not None and _table(guards.class_dog, c) and bool(np.float32(x) > np.float32(guards.dog_threshold))


def dog_drops(guards, c, d, v):
    """An event of class c due at d, v the largest dog-hit window before d (-1: none)."""
    return _table(guards.class_dog_filtered, c) and 0 <= v < d and d - v <= int(guards.dog_remember_windows)


def in_daylight(guards, c, b, spans):
    return _table(guards.class_daylight, c) and any(lo <= b < hi for lo, hi in spans)


def events(rows, flt, ext, guards):
    """-> the events (EVENT), ascending by (recording, class_index, first_window)."""
    if guards is None:
        return evxref.events(rows, flt, ext)
    hold = int(flt.hold_windows)
    every = types.SimpleNamespace(class_threshold=flt.class_threshold, class_veto=flt.class_veto, veto_threshold=flt.veto_threshold,
                                  hold_windows=flt.hold_windows, min_count=flt.min_count, flags=int(flt.flags) | KEEP_DROPPED)
    barks = {}
    for r, w, c, x in zip(rows["recording"].tolist(), rows["window"].tolist(), rows["class_index"].tolist(), rows["confidence"]):
        if dog_hit(guards, c, x):
            barks.setdefault(r, []).append(w)
    spans = {}
    for r, lo, hi in (() if guards.daylight_spans is None else np.asarray(guards.daylight_spans).reshape(-1, 3).tolist()):
        spans.setdefault(r, []).append((lo, hi))
    out = []
    for e in evxref.events(rows, every, ext).tolist():
        r, c, b, last, status = e[0], e[1], e[2], e[3], e[7]
        if status == KEPT:
            d = deadline(b, last, hold, ext) if slides(ext, c) else b + hold      # the final deadline: the last hit's stands
            v = max([w for w in barks.get(r, ()) if w < d], default=-1)
            if dog_drops(guards, c, d, v):
                status = DOG
            elif in_daylight(guards, c, b, spans.get(r, ())):
                status = DAYLIGHT
        if status == KEPT or (int(flt.flags) & KEEP_DROPPED):
            out.append(tuple(e[:7]) + (status,))
    return np.array(out, EVENT) if out else np.zeros(0, EVENT)


class _Source(evbankref._Source):
    def __init__(self):
        super().__init__()
        self.dog = -1

    def copy(self):
        c = _Source()
        c.clock, c.live, c.veto, c.dog = self.clock, {k: list(v) for k, v in self.live.items()}, self.veto, self.dog
        return c


class EventBank(evxref.EventBank):
    """evxref.EventBank (ext None: no class slides) under guards: a source also keeps its latest dog-hit window - recorded only while
    guards with a class_dog table are set, kept across flush and set_guards(None), cleared by reset - and the bank the sources'
    daylight spans.  A live event is [first, last, best, count, conf, deadline]."""

    def __init__(self, max_sources, n_classes, k, flt, ext=None, guards=None):
        super().__init__(max_sources, n_classes, k, flt, ext)
        self.day = {}
        self.set_guards(guards)

    def set_guards(self, guards):
        if guards is not None and int(guards.dog_remember_windows) < 0:
            raise ValueError("dog_remember_windows must not be negative")
        self.guards = guards

    def set_daylight(self, source, spans=()):
        spans = [(int(lo), int(hi)) for lo, hi in spans]
        if len(spans) > DAYLIGHT_SPANS or any(not 0 <= lo < hi for lo, hi in spans) or any(a[1] > b[0] for a, b in zip(spans, spans[1:])):
            raise ValueError("at most 8 spans, ascending and disjoint, 0 <= from < to")
        if source < 0:
            if spans:
                raise ValueError("source -1 only clears")
            self.day = {}
        else:
            self.day[source] = spans

    def _guarded(self, s, S, c, e):
        status = self._status(S, e)
        g = self.guards
        if status == KEPT and g is not None:
            if dog_drops(g, c, e[5], S.dog):                             # from the final deadline, which an early flush has not reached
                status = DOG
            elif in_daylight(g, c, e[0], self.day.get(s, ())):
                status = DAYLIGHT
        return status

    def process(self, sources, conf, idx, cap=None):
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
                if dog_hit(self.guards, c, x):                           # whatever else the result is
                    S.dog = w
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
                out.append((s, c, e[0], e[1], e[2], e[3], e[4], self._guarded(s, S, c, e)))
            S.clock = w + 1
        out = self._answer(out, cap)
        self.src.update(work)                                            # the commit: nothing changed before here, no dog window either
        return out

    def flush(self, source=-1, cap=None):
        which = sorted(self.src) if source < 0 else [source] if source in self.src else []
        out = [(s, c, e[0], e[1], e[2], e[3], e[4], self._guarded(s, self.src[s], c, e)) for s in which for c, e in self.src[s].live.items()]
        out = self._answer(out, cap)
        for s in which:
            self.src[s].live = {}
        return out

    def reset(self, source=-1):
        super().reset(source)
        if source < 0:
            self.day = {}
        else:
            self.day.pop(source, None)
