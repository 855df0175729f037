"""Detection events without a device: the restatement of the rule (tests/evref.py) against a second, independent statement of it,
the host-only entry bnhip_event_min_count, wav.EventFilter's tables, and every refusal of the events entries."""
import ctypes as C
import math

import numpy as np
import pytest

from birdnet_go_amd import host, wav

import evref


# ------------------------------------------------------------------------------------------ the rule, stated twice
def _go_processor(rows, flt):
    """The reference's processor fed window by window in audio time: a pending map keyed by (source, species) with a flush deadline
    (created + hold), a count and best-on->; the last human time of a source, compared at the flush with !Before(FirstDetected)."""
    thr = np.asarray(flt.class_threshold, np.float32)
    veto = np.zeros(thr.size, np.uint8) if flt.class_veto is None else np.asarray(flt.class_veto, np.uint8)
    done = []
    by_source = {}
    for q in rows:
        by_source.setdefault(int(q["recording"]), {}).setdefault(int(q["window"]), []).append((int(q["class_index"]), np.float32(q["confidence"])))
    for source, ticks in by_source.items():
        pending, last_human = {}, None

        def flush(now):
            for species in [s for s, p in pending.items() if now is None or now >= p["deadline"]]:
                p = pending.pop(species)
                if p["count"] < flt.min_count:                              # shouldDiscardDetection
                    status = 1
                elif last_human is not None and not last_human < p["first"]:    # !LastHumanDetection.Before(FirstDetected)
                    status = 2
                else:
                    status = 0
                done.append((source, species, p["first"], p["last"], p["best"], p["count"], p["conf"], status))

        for now in range(max(ticks) + 1):
            flush(now)
            for species, conf in ticks.get(now, ()):
                if veto[species]:
                    if conf > np.float32(flt.veto_threshold):
                        last_human = now                                    # handleHumanDetection
                    continue
                if conf <= thr[species] or math.isnan(conf) or math.isnan(thr[species]):     # result.Confidence <= confidenceThreshold
                    continue
                p = pending.get(species)
                if p is None:
                    pending[species] = {"first": now, "last": now, "best": now, "count": 1, "conf": conf, "deadline": now + flt.hold_windows}
                    continue
                if conf > p["conf"]:
                    p["conf"], p["best"] = conf, now
                p["count"] += 1
                p["last"] = now
        flush(None)
    if not (flt.flags & evref.KEEP_DROPPED):
        done = [e for e in done if e[-1] == 0]
    done.sort(key=lambda e: e[:3])
    return np.array(done, evref.EVENT) if done else np.zeros(0, evref.EVENT)


def _random_rows(rng, n, n_rec, n_classes, n_windows):
    rows = np.zeros(n, host.DETECTION)
    rows["recording"] = rng.integers(0, n_rec, n)
    rows["window"] = rng.integers(0, n_windows, n)
    rows["class_index"] = rng.integers(0, n_classes, n)
    rows["confidence"] = (rng.integers(0, 64, n) / 64.0).astype(np.float32)        # few values: ties and == threshold happen
    rows["confidence"][rng.integers(0, n, n // 50)] = np.nan
    return rows[np.lexsort((rows["window"], rows["recording"]))]


@pytest.mark.parametrize("hold", [1, 2, 7])
@pytest.mark.parametrize("min_count", [1, 2, 3, 4])
def test_restatement_is_the_processor(hold, min_count):
    rng = np.random.default_rng(1000 * hold + min_count)
    rows = _random_rows(rng, 3000, 5, 40, 60)
    thr = (rng.integers(8, 56, 40) / 64.0).astype(np.float32)
    thr[3], thr[4] = np.inf, np.nan
    veto = np.zeros(40, np.uint8)
    veto[[7, 21]] = 1
    for flags in (0, evref.KEEP_DROPPED):
        flt = host.EventTables(thr, veto, 0.9, hold, min_count, flags)
        want, got = _go_processor(rows, flt), evref.events(rows, flt)
        assert (got.size or not flags) and np.array_equal(got, want)
        if flags and hold == 7 and min_count == 2:
            assert set(got["status"]) == {0, 1, 2}                              # (of the input: the comparison sees every status)
    assert host.EVENT == evref.EVENT


# ------------------------------------------------------------------------------------------ bnhip_event_min_count
def test_min_count_by_hand(built_lib):
    lib = host._analyze_events_protos(host.load_library())
    for level, overlap, want in [(0, 0.0, 1), (0, 2.5, 1), (0, 2.95, 1), (3, 2.0, 3), (1, 2.5, 3), (5, 2.5, 9), (3, 2.95, 30), (5, 0.0, 2),
                                 (2, 2.0, 2), (7, 2.0, 2), (-1, 2.0, 2)]:
        assert lib.bnhip_event_min_count(level, overlap) == want, (level, overlap)
        assert host.event_min_count(level, overlap) == want


# ------------------------------------------------------------------------------------------ wav.EventFilter
def test_event_filter_tables(built_lib):
    f = wav.EventFilter(default_threshold=0.7, thresholds={2: 0.1, 5: 0.95}, include=[1, 2, 5, 6], exclude=[6], veto=[0], veto_threshold=0.3,
                        hold_seconds=15.0, level=3, keep_dropped=True)
    t = f.tables(8, 48000, 24000, overlap_seconds=2.5)
    assert t.class_threshold.dtype == np.float32 and t.class_veto.tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    assert np.isinf(t.class_threshold[[0, 3, 4, 6, 7]]).all()
    # 0.7, 0.1, 0.95 and 0.3 are not float32 values: each table entry is the float32 below, so `x > entry` is `x > value` for every
    # float32 x - the neighbour above the entry already exceeds the value
    for j, v in [(1, 0.7), (2, 0.1), (5, 0.95)]:
        e = t.class_threshold[j]
        assert float(e) < v < float(np.nextafter(e, np.float32(np.inf)))
    assert float(np.float32(0.1)) > 0.1 and t.class_threshold[2] == np.nextafter(np.float32(0.1), np.float32(-np.inf))     # nearest lies above
    assert float(np.float32(0.7)) < 0.7 and t.class_threshold[1] == np.float32(0.7)                                       # nearest lies below
    assert wav.EventFilter(default_threshold=0.5).tables(3, 48000, 48000).class_threshold.tolist() == [0.5] * 3             # representable: kept
    assert float(np.float32(t.veto_threshold)) == t.veto_threshold <= 0.3
    assert t.hold_windows == 30 and t.min_count == 6 and t.flags == host.EVENTS_KEEP_DROPPED       # 15 s at a 0.5 s hop; level 3 at 2.5 s: 12 * 0.5
    assert wav.EventFilter(hold_seconds=1.0).hold_windows(48000, 144000) == 1
    assert wav.EventFilter(hold_seconds=15.0).hold_windows(48000, 144000) == 5
    assert wav.EventFilter(hold_seconds=15.1).hold_windows(48000, 144000) == 6
    plain = wav.EventFilter(min_count=2).tables(4, 48000, 48000)
    assert plain.class_veto is None and plain.min_count == 2 and plain.flags == 0
    assert (plain.class_threshold == np.nextafter(np.float32(0.8), np.float32(-np.inf))).all() and float(np.float32(0.8)) > 0.8
    with pytest.raises(ValueError):
        wav.EventFilter(min_count=2, level=1)


# ------------------------------------------------------------------------------------------ refusals
def _refused(lib, rc):
    return rc == host.E_INVALID and len(lib.bnhip_last_error()) > 0


def test_stand_alone_entry_refuses(built_lib):
    """bnhip_detection_events: one invalid argument per call, BNHIP_E_INVALID with a text, nothing written, no device needed."""
    lib = host._analyze_events_protos(host.load_library())
    P = lambda a: a.ctypes.data
    rows = np.zeros(4, host.DETECTION)
    rows["window"], rows["class_index"], rows["confidence"] = [0, 1, 1, 2], [0, 1, 2, 3], 0.9
    thr = np.full(4, 0.5, np.float32)
    out = np.zeros(4, host.EVENT)
    out["count"] = -7
    n_out = C.c_size_t(12345)

    def call(rows=rows, n=None, n_classes=4, thr=P(thr), hold=3, min_count=1, flags=0, flt=True, o=P(out), cap=4, no=C.byref(n_out)):
        fs = host._EventFilterStruct(thr, None, 0.5, hold, min_count, flags)
        return lib.bnhip_detection_events(0, P(rows) if rows is not None else None, rows.size if n is None else n, n_classes,
                                          C.addressof(fs) if flt else None, o, cap, no)

    def edit(field, i, v):
        r = rows.copy()
        r[field][i] = v
        return r

    cases = [dict(flt=False), dict(thr=None), dict(hold=0), dict(min_count=0), dict(flags=2), dict(flags=-1), dict(n_classes=0),
             dict(n_classes=38401), dict(rows=edit("recording", 3, 65535)), dict(rows=edit("recording", 0, -1)), dict(rows=edit("window", 0, -1)),
             dict(rows=edit("class_index", 2, 4)), dict(rows=edit("class_index", 2, -1)), dict(rows=edit("window", 2, 0)),
             dict(rows=edit("recording", 1, 1)), dict(n=1 << 31), dict(no=None), dict(o=None), dict(rows=None, n=4)]
    for kw in cases:
        assert _refused(lib, call(**kw)), kw
    assert (out["count"] == -7).all() and n_out.value == 12345
    # no rows: zero events, and still no device
    assert call(n=0) == host.BNHIP_OK and n_out.value == 0
    assert _refused(lib, call(n=0, hold=0))


def test_fused_entries_refuse(built_lib, tiny_blob):
    """bnhip_analyze_*_pcm_events on a plan-only handle: what the sibling refuses and what the filter adds, each before the handle is
    looked at; a well-formed call is refused for the handle."""
    lib = host._analyze_events_protos(host.load_library())
    m = host.HipClassifier(tiny_blob, plan_only=True)
    try:
        n, nc = m.n_samples, m.num_species()
        P = lambda a: a.ctypes.data
        pcm = np.zeros(4 * n, np.int16)
        ln = np.array([2 * n], np.int64)
        recs = host.recordings([2 * n], 48000, 16)
        mixed = host.recordings([2 * n], 32000, 16)
        crecs = host.channel_recordings([2 * n], 48000, 16, 2, "mix")
        thr = np.full(nc, 0.5, np.float32)
        out = np.zeros(15, host.EVENT)
        out["count"] = -7
        n_out = C.c_size_t(12345)
        chosen = np.full(1, -7, np.int32)

        def flt(thr=P(thr), hold=3, min_count=1, flags=0):
            return host._EventFilterStruct(thr, None, 0.5, hold, min_count, flags)

        def plain(fs=flt(), null=False, bits=16, nr=1, hop=n // 2, k=5, o=P(out), cap=15, no=C.byref(n_out)):
            return lib.bnhip_analyze_pcm_events(m._h, P(pcm), bits, P(ln), nr, hop, 0, 0, 1.0, k, None if null else C.addressof(fs), o, cap, no)

        def mix(fs=flt(), null=False, table=recs, rate=48000, nr=1, hop=n // 2, k=5, o=P(out), cap=15, no=C.byref(n_out)):
            return lib.bnhip_analyze_mixed_pcm_events(m._h, P(pcm), P(table), nr, rate, hop, 0, 0, 1.0, k, None if null else C.addressof(fs), o, cap, no)

        def chan(fs=flt(), null=False, table=crecs, rate=48000, nr=1, hop=n // 2, k=5, o=P(out), cap=15, no=C.byref(n_out)):
            return lib.bnhip_analyze_channels_pcm_events(m._h, P(pcm), P(table), nr, rate, hop, 0, 0, 1.0, k, None if null else C.addressof(fs), o, cap,
                                                         no, P(chosen))

        bad_filters = [dict(null=True), dict(fs=flt(thr=None)), dict(fs=flt(hold=0)), dict(fs=flt(min_count=0)), dict(fs=flt(flags=2))]
        bad_depth = host.recordings([2 * n], 48000, 8)
        bad_channels = host.channel_recordings([2 * n], 48000, 16, 17, "mix")
        assert mix(table=mixed) == host.E_INVALID and b"plan-only" in lib.bnhip_last_error()       # (the resampling route: well-formed too)
        for f, more in [(plain, [dict(bits=8)]), (mix, [dict(table=bad_depth), dict(rate=0)]), (chan, [dict(table=bad_channels), dict(rate=0)])]:
            assert f() == host.E_INVALID and b"plan-only" in lib.bnhip_last_error()
            for kw in bad_filters + more + [dict(nr=0), dict(hop=0), dict(hop=n + 1), dict(k=0), dict(no=None), dict(o=None)]:
                assert _refused(lib, f(**kw)), (f.__name__, kw)
                assert b"plan-only" not in lib.bnhip_last_error(), (f.__name__, kw)
        assert (out["count"] == -7).all() and n_out.value == 12345 and chosen[0] == -7
        assert m.describe()["n_samples"] == n
    finally:
        m.close()


def test_row_bound_is_refused_before_the_handle(built_lib, tiny_blob):
    """windows * min(k, n_classes) >= 2^31, from the window table alone: one long recording at hop 1."""
    lib = host._analyze_events_protos(host.load_library())
    m = host.HipClassifier(tiny_blob, plan_only=True)
    try:
        n, nc = m.n_samples, m.num_species()
        k = min(nc, 8)
        windows = -(-(1 << 31) // k)
        ln = np.array([n + (windows - 1)], np.int64)                          # hop 1: one window per sample behind the first clip
        assert host.analyze_windows(ln, n, 1)[-1] == windows
        thr = np.zeros(nc, np.float32)
        fs = host._EventFilterStruct(thr.ctypes.data, None, 0.5, 1, 1, 0)
        n_out = C.c_size_t(12345)
        dummy = np.zeros(16, np.int16)                                       # never read: the call is refused before any copy
        rc = lib.bnhip_analyze_pcm_events(m._h, dummy.ctypes.data, 16, ln.ctypes.data, 1, 1, 0, 0, 1.0, k, C.addressof(fs), None, 0, C.byref(n_out))
        assert _refused(lib, rc) and b"2^31 detection rows" in lib.bnhip_last_error() and n_out.value == 12345
    finally:
        m.close()
