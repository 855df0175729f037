"""The real-time event bank without a device: the streaming restatement (tests/evbankref.py) against the one-shot rule
(tests/evref.py) and the reference's processor fed window by window, when every event is answered, and every refusal of the bank's
entries that needs no device."""
import ctypes as C

import numpy as np
import pytest

from birdnet_go_amd import host

import evbankref
import evref
from test_analyze_events_ref import _go_processor


def topk_rows(rng, n_src, n_win, n_classes, k, nan_share=0.02, empty_share=0.15):
    """-> conf, idx [n_src, n_win, k]: per window k distinct classes (some entries -1: no result), few confidence values so that ties and
    == threshold happen, a few NaN; some windows wholly empty."""
    conf = (rng.integers(0, 64, (n_src, n_win, k)) / 64.0).astype(np.float32)
    conf[rng.random(conf.shape) < nan_share] = np.nan
    idx = np.stack([[rng.permutation(n_classes)[:k] for _ in range(n_win)] for _ in range(n_src)]).astype(np.int32)
    idx[rng.random(idx.shape) < 0.1] = -1
    idx[rng.random((n_src, n_win)) < empty_share] = -1
    return conf, idx


def detection_rows(conf, idx):
    """The same results as the DETECTION rows of a file-analysis call: by recording, window, rank; no-results left out."""
    s, w, r = np.nonzero(idx >= 0)
    rows = np.zeros(s.size, host.DETECTION)
    rows["recording"], rows["window"], rows["class_index"], rows["confidence"] = s, w, idx[s, w, r], conf[s, w, r]
    return rows


def by_key(events):
    ev = np.concatenate(events) if len(events) else np.zeros(0, evref.EVENT)
    return ev[np.lexsort((ev["first_window"], ev["class_index"], ev["recording"]))]


def feed(bank, conf, idx, plan, rng=None):
    """Feeds every source's windows in order under `plan` ("window": one window of every source per call; "all": one call, the rows
    interleaved at random; "groups": random numbers of windows of random sources per call) -> [(answer, {source: (first, last window
    applied)})] per call."""
    n_src, n_win, k = conf.shape
    at = [0] * n_src
    calls = []
    while any(a < n_win for a in at):
        if plan == "window":
            take = [(s, 1) for s in range(n_src)]
        elif plan == "all":
            take = [(s, n_win) for s in range(n_src)]
        else:
            take = [(s, int(rng.integers(1, 5))) for s in range(n_src) if rng.random() < 0.6]
        rows = [(s, at[s] + j) for s, n in take for j in range(min(n, n_win - at[s]))]
        if plan != "window" and rng is not None:                       # any interleaving that keeps each source's order
            keys = np.argsort(rng.random(len(rows)), kind="stable")
            nxt, order = {s: at[s] for s in range(n_src)}, []
            for i in keys:
                s = rows[i][0]
                order.append((s, nxt[s]))
                nxt[s] += 1
            rows = order
        span = {}
        for s, w in rows:
            span[s] = (min(span.get(s, (w, w))[0], w), max(span.get(s, (w, w))[1], w))
            at[s] = max(at[s], w + 1)
        src = [s for s, _ in rows]
        got = bank.process(src, np.array([conf[s, w] for s, w in rows]).reshape(len(rows), k), np.array([idx[s, w] for s, w in rows]).reshape(len(rows), k))
        calls.append((got, span))
    return calls


def filters(rng, n_classes, hold, min_count, veto, flags):
    thr = (rng.integers(8, 56, n_classes) / 64.0).astype(np.float32)
    thr[1], thr[2] = np.inf, np.nan
    v = None
    if veto:
        v = np.zeros(n_classes, np.uint8)
        v[[0, n_classes // 2]] = 1
    return host.EventTables(thr, v, 0.6, hold, min_count, flags)


@pytest.mark.parametrize("hold", [1, 3, 8])
@pytest.mark.parametrize("min_count", [1, 3])
@pytest.mark.parametrize("veto", [False, True])
def test_streaming_rule_is_the_one_shot_rule(hold, min_count, veto):
    saw = set()
    for seed in range(3):
        for flags in (0, evref.KEEP_DROPPED):
            rng = np.random.default_rng(1000 * hold + 100 * min_count + 10 * seed + veto)
            n_src, n_win, n_classes, k = 3, 40, 12, 4
            conf, idx = topk_rows(rng, n_src, n_win, n_classes, k)
            flt = filters(rng, n_classes, hold, min_count, veto, flags)
            rows = detection_rows(conf, idx)
            want = evref.events(rows, flt)
            assert (want.size or not flags) and np.array_equal(want, _go_processor(rows, flt))
            saw |= set(want["status"].tolist())
            for plan in ("window", "all", "groups"):
                bank = evbankref.EventBank(n_src, n_classes, k, flt)
                calls = feed(bank, conf, idx, plan, np.random.default_rng(seed))
                tail = bank.flush()
                assert bank.pending().size == 0 and [bank.clock(s) for s in range(n_src)] == [n_win] * n_src
                got = by_key([c[0] for c in calls] + [tail])
                assert np.array_equal(got, want), (plan, seed, flags)
                # every event is answered in the call that applies window first_window + hold - 1, or in the flush
                for ans, span in calls:
                    assert np.array_equal(ans, by_key([ans]))                   # a call's own answer is in key order
                    for e in ans:
                        lo, hi = span[int(e["recording"])]
                        assert lo <= e["first_window"] + hold - 1 <= hi
                assert (tail["first_window"] + hold - 1 >= n_win).all()
    if hold == 8:                                                                # (of the input: the comparison sees every status)
        assert saw == ({0, 1, 2} if veto and min_count > 1 else {0, 2} if veto else {0, 1} if min_count > 1 else {0})


def test_restatement_entries():
    """pending, reset, set_filter, a refused call and the slot bound of the restatement itself."""
    rng = np.random.default_rng(5)
    flt = filters(rng, 12, 4, 1, False, 0)
    conf, idx = topk_rows(rng, 2, 10, 12, 4, empty_share=0.0)
    bank = evbankref.EventBank(2, 12, 4, flt)
    assert bank.slots_per_source == 12 and evbankref.EventBank(2, 100, 4, flt).slots_per_source == 16
    feed(bank, conf[:, :5], idx[:, :5], "window")
    p = bank.pending()
    assert p.size and (p["status"] == evbankref.PENDING).all() and np.array_equal(p, by_key([p])) and np.array_equal(p, bank.pending())
    assert max(len(S.live) for S in bank.src.values()) <= bank.slots_per_source
    with pytest.raises(evbankref.TooSmall) as ei:
        bank.flush(cap=p.size - 1)
    assert ei.value.needed == p.size and np.array_equal(bank.pending(), p)      # nothing changed
    bank.reset(0)
    assert bank.clock(0) == 0 and bank.clock(1) == 5 and set(bank.pending()["recording"]) == {1}
    with pytest.raises(ValueError):
        bank.set_filter(host.EventTables(flt.class_threshold, None, 0.6, 5, 1, 0))
    bank.set_filter(host.EventTables(np.full(12, np.inf, np.float32), None, 0.6, 4, 1, 0))
    for w in range(5, 10):
        bank.process([1], conf[1, w], idx[1, w])
    assert bank.clock(1) == 10 and bank.pending().size == 0                                              # no class hits any more; the old events ran out


# ------------------------------------------------------------------------------------------ the library, no device
def test_symbols_and_refusals(built_lib):
    lib = host._event_bank_protos(host.load_library())
    for name in host.SYMBOLS:
        if "event_bank" in name or name == "bnhip_windows_predict_events":
            assert getattr(lib, name).argtypes is not None, name
    assert host.EVENT_PENDING == evbankref.PENDING == -1
    thr = np.full(8, 0.5, np.float32)
    h = C.c_void_p()

    def create(max_sources=4, n_classes=8, k=3, thr=thr.ctypes.data, hold=5, min_count=1, flags=0, flt=True, out=C.byref(h)):
        fs = host._EventFilterStruct(thr, None, 0.5, hold, min_count, flags)
        return lib.bnhip_event_bank_create(0, max_sources, n_classes, k, C.addressof(fs) if flt else None, out)

    for kw, text in [(dict(out=None), b"NULL"), (dict(flt=False), b"NULL"), (dict(thr=None), b"NULL"), (dict(max_sources=0), b"max_sources"),
                     (dict(max_sources=65536), b"max_sources"), (dict(n_classes=0), b"n_classes"), (dict(n_classes=38401), b"n_classes"),
                     (dict(k=0), b"k must be"), (dict(hold=0), b"hold_windows"), (dict(min_count=0), b"min_count"),
                     (dict(k=64, hold=65), b"k * hold_windows"), (dict(k=4097, hold=1), b"k * hold_windows"), (dict(flags=2), b"flags"),
                     (dict(flags=-1), b"flags")]:
        h.value = 12345
        assert create(**kw) == host.E_INVALID, kw
        assert text in lib.bnhip_last_error(), (kw, lib.bnhip_last_error())
        assert "out" in kw or h.value is None, kw
    # a NULL bank, or no place for the answer
    n, ev, w = C.c_size_t(777), np.zeros(2, host.EVENT), C.c_int64(5)
    fs = host._EventFilterStruct(thr.ctypes.data, None, 0.5, 5, 1, 0)
    for rc in (lib.bnhip_event_bank_process(None, None, 0, None, None, ev.ctypes.data, 2, C.byref(n)),
               lib.bnhip_event_bank_process_device(None, None, 0, None, None, ev.ctypes.data, 2, C.byref(n), None),
               lib.bnhip_event_bank_flush(None, -1, ev.ctypes.data, 2, C.byref(n)), lib.bnhip_event_bank_pending(None, ev.ctypes.data, 2, C.byref(n)),
               lib.bnhip_event_bank_reset(None, -1), lib.bnhip_event_bank_clock(None, 0, C.byref(w)), lib.bnhip_event_bank_set_filter(None, C.addressof(fs)),
               lib.bnhip_event_bank_info(None, None, None, None, None, None),
               lib.bnhip_windows_predict_events(None, None, None, 16, 0, 1.0, 10, None, None, None, None, None, None, 0, None)):
        assert rc == host.E_INVALID and b"NULL" in lib.bnhip_last_error()
    assert n.value == 777 and w.value == 5
    lib.bnhip_event_bank_destroy(None)
