"""Extended capture without a device: the sliding deadline against a literal table of the reference's cases, the streaming
restatement (tests/evxref.py) against the one-shot one and both against evref where no class slides, every refusal of the extended
entries that needs no device, and wav.ExtendedCapture's seconds in windows."""
import ctypes as C

import numpy as np
import pytest

from birdnet_go_amd import host, wav

import evref
import evxref
from test_event_bank_ref import by_key, detection_rows, feed, filters, topk_rows

# the reference's constants in windows of 1 s (extended_capture.go: 15 s, 30 s / 30 s, 2 min / 60 s)
REF = dict(short_wait=15, medium_from=30, medium_wait=30, long_from=120, long_wait=60)
# the small numbers of the device tests: every stage inside 14 windows
SMALL = dict(max_windows=14, short_wait=2, medium_from=5, medium_wait=4, long_from=9, long_wait=6)


def extend(table=None, **kw):
    return host.EventExtend(table, **kw)


# (normal window, MaxDuration, first hit, hit) -> deadline: calculateExtendedFlushDeadline by hand
DEADLINES = [
    (12, 600, 100, 100, 115),        # session 0 s, normal window below 15 s: now + 15
    (12, 600, 100, 129, 144),        # 29 s: still short
    (12, 600, 100, 130, 160),        # 30 s: now + 30
    (12, 600, 100, 219, 249),        # 119 s: still medium
    (12, 600, 100, 220, 280),        # 120 s: now + 60
    (20, 600, 100, 100, 120),        # normal window above 15 s: now + 20
    (20, 600, 100, 129, 149),
    (20, 600, 100, 130, 160),        # ... which the medium stage does not look at
    (20, 600, 100, 220, 280),
    (12, 600, 100, 650, 700),        # the cap: FirstDetected + MaxDuration, not now + 60
    (12, 600, 100, 640, 700),        # ... reached exactly
    (12, 600, 100, 639, 699),
    (12, 40, 100, 124, 139),
    (12, 40, 100, 125, 140),
    (12, 40, 100, 129, 140),         # capped while still short
    (12, 12, 0, 0, 12),              # MaxDuration == the normal window: the fixed hold
]


@pytest.mark.parametrize("hold,most,b,w,want", DEADLINES)
def test_deadline_table(built_lib, hold, most, b, w, want):
    x = extend(max_windows=most, **REF)
    assert evxref.deadline(b, w, hold, x) == want
    assert host.event_deadline(hold, x, b, w) == want


def test_deadline_library_is_restatement(built_lib):
    for hold in (1, 3, 8):
        x = extend(**SMALL)
        for b in (0, 7):
            for w in range(b, b + 20):
                assert host.event_deadline(hold, x, b, w) == evxref.deadline(b, w, hold, x) >= min(w + 1, b + 14)
    with pytest.raises(host.HipError):
        host.event_deadline(3, extend(**SMALL), 5, 4)


def mixed_table(rng, n_classes):
    t = (rng.random(n_classes) < 0.5).astype(np.uint8)
    t[3], t[4] = 1, 0
    return t


@pytest.mark.parametrize("hold", [1, 3, 8])
@pytest.mark.parametrize("min_count", [1, 3])
def test_streaming_rule_is_the_one_shot_rule(hold, min_count):
    longest = 0
    for seed in range(3):
        for flags in (0, evref.KEEP_DROPPED):
            rng = np.random.default_rng(1000 * hold + 100 * min_count + 10 * seed)
            n_src, n_win, n_classes, k = 3, 40, 12, 4
            conf, idx = topk_rows(rng, n_src, n_win, n_classes, k)
            flt = filters(rng, n_classes, hold, min_count, True, flags)
            x = extend(mixed_table(rng, n_classes), **SMALL)
            rows = detection_rows(conf, idx)
            want = evxref.events(rows, flt, x)
            assert want.size or not flags
            fixed = want[x.class_extended[want["class_index"]] == 0]
            assert ((fixed["last_window"] - fixed["first_window"]) < hold).all()
            assert ((want["last_window"] - want["first_window"]) < 14).all()
            longest = max(longest, int((want["last_window"] - want["first_window"]).max()) if want.size else 0)
            for plan in ("window", "all", "groups"):
                bank = evxref.EventBank(n_src, n_classes, k, flt, x)
                assert bank.slots_per_source == min(k * max(hold, 6), n_classes)
                calls = feed(bank, conf, idx, plan, np.random.default_rng(seed))
                assert max(len(S.live) for S in bank.src.values()) <= bank.slots_per_source
                tail = bank.flush()
                assert bank.pending().size == 0
                assert np.array_equal(by_key([c[0] for c in calls] + [tail]), want), (plan, seed, flags)
    assert longest >= hold                                               # (of the input: an event no fixed hold could give)


@pytest.mark.parametrize("hold", [1, 3, 8])
def test_no_sliding_class_is_the_fixed_rule(hold):
    rng = np.random.default_rng(hold)
    n_src, n_win, n_classes, k = 3, 40, 12, 4
    conf, idx = topk_rows(rng, n_src, n_win, n_classes, k)
    rows = detection_rows(conf, idx)
    for flags in (0, evref.KEEP_DROPPED):
        flt = filters(rng, n_classes, hold, 2, True, flags)
        want = evref.events(rows, flt)
        for x in (extend(np.zeros(n_classes, np.uint8), **SMALL), None):
            assert np.array_equal(evxref.events(rows, flt, x), want)
            bank = evxref.EventBank(n_src, n_classes, k, flt, x)
            calls = feed(bank, conf, idx, "groups", np.random.default_rng(1))
            assert np.array_equal(by_key([c[0] for c in calls] + [bank.flush()]), want)
        # (of the input: with every class sliding the same rows merge differently)
        assert not np.array_equal(evxref.events(rows, flt, extend(max_windows=40, short_wait=9, medium_from=20, medium_wait=9, long_from=30,
                                                                  long_wait=9)), want)


def test_restatement_set_extend():
    """A live event keeps its deadline until its next hit; None turns sliding off; a larger W is refused."""
    n_classes, k, hold = 6, 2, 3
    flt = host.EventTables(np.full(n_classes, 0.5, np.float32), None, 0.5, hold, 1, 0)
    bank = evxref.EventBank(1, n_classes, k, flt, extend(**SMALL))
    hit = lambda *cls: (np.full((1, k), 0.75, np.float32), np.array([list(cls) + [-1] * (k - len(cls))], np.int32))
    bank.process([0], *hit(1, 2))                                        # window 0: deadlines 3
    bank.set_extend(None)
    bank.process([0], *hit(1))                                           # window 1: class 1 joins, no slide; class 2 untouched
    assert bank.process([0], *hit()).size == 2                           # window 2: both due at 3
    bank.set_extend(extend(**SMALL))
    bank.process([0], *hit(1))                                           # window 3 opens: deadline 6
    bank.process([0], *hit(1))                                           # window 4 slides it to 7
    assert bank.src[0].live[1][5] == 7
    with pytest.raises(ValueError):
        bank.set_extend(extend(**dict(SMALL, long_wait=7)))


# ------------------------------------------------------------------------------------------ the library, no device
def test_symbols_and_refusals(built_lib):
    lib = host._event_bank_protos(host.load_library())
    for name in ("bnhip_detection_events_extended", "bnhip_analyze_channels_pcm_events_extended", "bnhip_analyze_channels_pcm_clips_extended",
                 "bnhip_event_bank_create_extended", "bnhip_event_bank_set_extend", "bnhip_event_deadline"):
        assert name in host.SYMBOLS and getattr(lib, name) is not None, name
    thr = np.full(8, 0.5, np.float32)
    h = C.c_void_p()
    fs = host._EventFilterStruct(thr.ctypes.data, None, 0.5, 5, 1, 0)
    n, ev = C.c_size_t(777), np.zeros(2, host.EVENT)
    good = dict(max_windows=20, short_wait=2, medium_from=5, medium_wait=4, long_from=9, long_wait=6)

    def entries(k=3, null=False, **kw):
        xs = host._EventExtendStruct(None, *[dict(good, **kw)[f] for f in ("max_windows", "short_wait", "medium_from", "medium_wait",
                                                                            "long_from", "long_wait")])
        px = None if null else C.addressof(xs)
        return [lib.bnhip_event_bank_create_extended(0, 4, 8, k, C.addressof(fs), px, C.byref(h)),
                lib.bnhip_detection_events_extended(0, None, 0, 8, C.addressof(fs), px, ev.ctypes.data, 2, C.byref(n))]

    for kw, text in [(dict(null=True), b"NULL event extend"), (dict(max_windows=4), b"max_windows must be at least hold_windows"),
                     (dict(short_wait=0), b"short_wait must be at least 1"), (dict(medium_wait=0), b"medium_wait must be at least 1"),
                     (dict(long_wait=-3), b"long_wait must be at least 1"), (dict(medium_from=0), b"medium_from must be at least 1"),
                     (dict(long_from=4), b"long_from must be at least medium_from")]:
        h.value = 12345
        for rc in entries(**kw):
            assert rc == host.E_INVALID and text in lib.bnhip_last_error(), (kw, lib.bnhip_last_error())
        assert h.value is None and n.value == 777
    # k * W: the bank alone, and W is the longest of the four
    for kw in (dict(k=64, long_wait=65), dict(k=64, medium_wait=65), dict(k=64, short_wait=65), dict(k=683)):
        assert entries(**kw)[0] == host.E_INVALID and b"k * W must be at most 4096" in lib.bnhip_last_error(), kw
    assert entries(k=64, long_wait=65)[1] == host.BNHIP_OK and n.value == 0            # (the tail alone has no slots; no rows: no device)
    assert entries(k=820)[0] == host.E_INVALID and b"k * hold_windows" in lib.bnhip_last_error()       # hold 5: the filter's own bound first
    assert lib.bnhip_event_bank_set_extend(None, None) == host.E_INVALID and b"NULL" in lib.bnhip_last_error()
    # the Python layer: a table of another size
    with pytest.raises(host.HipError, match="n_classes"):
        host.detection_events(np.zeros(0, host.DETECTION), 8, host.EventTables(thr, None, 0.5, 5, 1, 0), extend=extend(np.zeros(7, np.uint8), **good))


def test_window_batcher_refuses_an_extend_it_would_ignore():
    """Banks exist on the native path and with events only: extend= without either is refused, as capture= is."""
    from birdnet_go_amd import stream as S
    flt = host.EventTables(np.full(8, 0.5, np.float32), None, 0.5, 5, 1, 0)
    for kw in (dict(events=None), dict(events=flt, native=False)):
        with pytest.raises(S.StreamError, match="extend needs events and the native rings"):
            S.WindowBatcher(S.Orchestrator(), extend=extend(**SMALL), **kw)


# ------------------------------------------------------------------------------------------ seconds to windows
@pytest.mark.parametrize("overlap,want", [(0.0, (34, 5, 10, 10, 40, 20)), (1.5, (67, 10, 20, 20, 80, 40)), (2.5, (200, 30, 60, 60, 240, 120))])
def test_extended_capture_tables(overlap, want):
    """48 kHz, 3 s clips: hops of 3 s, 1.5 s and 0.5 s; 100 s is no multiple of the first two: the ceiling, as hold_windows takes it."""
    rate, hop = 48000, int(round((3.0 - overlap) * 48000))
    x = wav.ExtendedCapture(species=[2, 5], max_seconds=100.0).tables(9, rate, hop)
    assert (x.max_windows, x.short_wait, x.medium_from, x.medium_wait, x.long_from, x.long_wait) == want
    assert x.class_extended.tolist() == [0, 0, 1, 0, 0, 1, 0, 0, 0] and x.class_extended.dtype == np.uint8
    assert wav.ExtendedCapture(max_seconds=100.0).tables(9, rate, hop).class_extended is None
    assert wav.EventFilter(hold_seconds=100.0).hold_windows(rate, hop) == want[0]
    other = wav.ExtendedCapture(None, 7.0, 0.1, 1.0, 2.0, 4.0, 8.0).tables(9, rate, hop)
    assert other.short_wait == 1 and other.long_wait == int(np.ceil(8.0 * rate / hop))
    with pytest.raises(ValueError):
        wav.ExtendedCapture()
