"""The detection-event rule (include/bnhip.h, "Detection events"), restated once in numpy and plain Python.  Everything else - the
device tail behind bnhip_analyze_*_pcm_events, bnhip_detection_events, wav.analyze_files(events=...) - is pinned to `events`.

rows: a structured array with the fields of bnhip_detection (recording, window, class_index, confidence), in the order
bnhip_analyze_pcm writes them.  The filter is any object with class_threshold, class_veto (or None), veto_threshold, hold_windows,
min_count and flags."""
import numpy as np

EVENT = np.dtype([("recording", "<i4"), ("class_index", "<i4"), ("first_window", "<i4"), ("last_window", "<i4"), ("best_window", "<i4"),
                  ("count", "<i4"), ("confidence", "<f4"), ("status", "<i4")])
KEEP_DROPPED = 1
KEPT, FEW, VETOED = 0, 1, 2


def marks(rows, flt):
    """-> (hits: {(recording, class): [(window, confidence), ...] in row order}, veto: {recording: set of windows})."""
    thr = np.asarray(flt.class_threshold, np.float32)
    veto = np.zeros(thr.size, np.uint8) if flt.class_veto is None else np.asarray(flt.class_veto, np.uint8)
    vt = np.float32(flt.veto_threshold)
    hits, vetoed = {}, {}
    for r, w, c, x in zip(rows["recording"].tolist(), rows["window"].tolist(), rows["class_index"].tolist(), rows["confidence"]):
        x = np.float32(x)
        if veto[c]:
            if x > vt:                                                   # float32, strict; false for a NaN on either side
                vetoed.setdefault(r, set()).add(w)
        elif x > thr[c]:
            hits.setdefault((r, c), []).append((w, x))
    return hits, vetoed


def events(rows, flt):
    """-> the events (EVENT), ascending by (recording, class_index, first_window)."""
    hold, min_count = int(flt.hold_windows), int(flt.min_count)
    hits, vetoed = marks(rows, flt)
    out = []
    for r, c in sorted(hits):
        group = sorted(hits[(r, c)], key=lambda h: h[0])                # stable: equal windows stay in row order
        found = []
        for w, x in group:
            if not found or w >= found[-1]["b"] + hold:                  # the hold counts from the event's first hit and does not slide
                found.append({"b": w, "last": w, "count": 1, "conf": x, "best": w})
                continue
            e = found[-1]
            e["last"], e["count"] = w, e["count"] + 1
            if x > e["conf"]:                                            # a tie keeps the earliest
                e["conf"], e["best"] = x, w
        for e in found:
            if e["count"] < min_count:
                status = FEW
            elif any(e["b"] <= v < e["b"] + hold for v in vetoed.get(r, ())):
                status = VETOED
            else:
                status = KEPT
            if status == KEPT or (int(flt.flags) & KEEP_DROPPED):
                out.append((r, c, e["b"], e["last"], e["best"], e["count"], e["conf"], status))
    return np.array(out, EVENT) if out else np.zeros(0, EVENT)
