"""The dog-bark and daylight filters without a device: the restatement (tests/guardref.py) against evxref where the guards do
nothing, its streaming form against its one-shot form, the edges of the rule worked by hand, and every refusal of the guarded
entries that needs no device."""
import ctypes as C

import numpy as np
import pytest

from birdnet_go_amd import host

import evref
import evxref
import guardref
from guardref import DAYLIGHT, DOG, FEW, KEPT, VETOED
from test_event_bank_ref import by_key, detection_rows, feed, filters, topk_rows
from test_event_extend_ref import SMALL, extend, mixed_table


def random_guards(rng, n_classes, n_rec, n_win, remember=3, n_dog=2, dog_threshold=0.7):
    """Guards that drop a visible share: n_dog dog classes (one also above its own threshold now and then, one a veto class of
    `filters`), half the classes filtered, half dropped in daylight, up to three spans per recording and none for the last."""
    dog = np.zeros(n_classes, np.uint8)
    dog[[0, 5, 7, 11, 13, 17, 19, 23][:n_dog]] = 1
    spans = []
    for r in range(n_rec - 1):
        edges = np.sort(rng.choice(np.arange(n_win + 4), 2 * int(rng.integers(1, 4)), replace=False))
        spans += [(r, int(lo), int(hi)) for lo, hi in edges.reshape(-1, 2)]
    return host.EventGuards(dog, dog_threshold, (rng.random(n_classes) < 0.5).astype(np.uint8), remember, (rng.random(n_classes) < 0.5).astype(np.uint8),
                            np.array(spans, np.int32).reshape(-1, 3))


def spans_of(guards, r):
    return [(lo, hi) for q, lo, hi in guards.daylight_spans.tolist() if q == r]


@pytest.mark.parametrize("hold", [1, 3])
def test_no_guards_is_the_rule_without(hold):
    rng = np.random.default_rng(hold)
    n_src, n_win, n_classes, k = 3, 40, 12, 4
    conf, idx = topk_rows(rng, n_src, n_win, n_classes, k)
    rows = detection_rows(conf, idx)
    zero = np.zeros(n_classes, np.uint8)
    for flags in (0, evref.KEEP_DROPPED):
        flt = filters(rng, n_classes, hold, 2, True, flags)
        for x in (None, extend(mixed_table(rng, n_classes), **SMALL)):
            want = evxref.events(rows, flt, x)
            for g in (None, host.EventGuards(), host.EventGuards(zero, 0.1, zero, 5, zero, None),
                      host.EventGuards(np.ones(n_classes, np.uint8), 0.0, None, 50, None, None)):       # (dog hits, but no species to drop)
                assert np.array_equal(guardref.events(rows, flt, x, g), want)
                bank = guardref.EventBank(n_src, n_classes, k, flt, x, g)
                calls = feed(bank, conf, idx, "groups", np.random.default_rng(1))
                assert np.array_equal(by_key([c[0] for c in calls] + [bank.flush()]), want)


@pytest.mark.parametrize("hold", [1, 3, 8])
@pytest.mark.parametrize("ext", [False, True])
def test_streaming_rule_is_the_one_shot_rule(hold, ext):
    saw, min_count = set(), 1 if hold == 1 else 2
    for seed in range(3):
        for flags in (0, evref.KEEP_DROPPED):
            rng = np.random.default_rng(100 * hold + 10 * seed + ext)
            n_src, n_win, n_classes, k = 3, 40, 12, 4
            conf, idx = topk_rows(rng, n_src, n_win, n_classes, k)
            flt = filters(rng, n_classes, hold, min_count, True, flags)
            x = extend(mixed_table(rng, n_classes), **SMALL) if ext else None
            g = random_guards(rng, n_classes, n_src, n_win)
            rows = detection_rows(conf, idx)
            want = guardref.events(rows, flt, x, g)
            saw |= set(want["status"].tolist())
            if not flags:
                every = guardref.events(rows, host.EventTables(flt.class_threshold, flt.class_veto, flt.veto_threshold, hold, min_count, 1), x, g)
                assert np.array_equal(want, every[every["status"] == KEPT])
            for plan in ("window", "all", "groups"):
                bank = guardref.EventBank(n_src, n_classes, k, flt, x, g)
                for s in range(n_src):
                    bank.set_daylight(s, spans_of(g, s))
                calls = feed(bank, conf, idx, plan, np.random.default_rng(seed))
                assert np.array_equal(by_key([c[0] for c in calls] + [bank.flush()]), want), (plan, seed, flags)
    assert saw == {KEPT, VETOED, DOG, DAYLIGHT} | ({FEW} if min_count > 1 else set())        # (of the input)


# ------------------------------------------------------------------------------------------ the edges, by hand
N, K, HOLD = 8, 2, 3
BIRD, OWL, DOGC, HUMAN = 1, 2, 6, 7                                      # thresholds 0.5; DOGC's own species threshold 0.8


def hand_filter(min_count=1, flags=evref.KEEP_DROPPED):
    thr = np.full(N, 0.5, np.float32)
    thr[DOGC] = 0.8
    veto = np.zeros(N, np.uint8)
    veto[HUMAN] = 1
    return host.EventTables(thr, veto, 0.5, HOLD, min_count, flags)


def hand_guards(remember=4, spans=None, filtered=(BIRD,), daylight=(OWL,)):
    t = lambda cs: np.isin(np.arange(N), cs).astype(np.uint8)
    return host.EventGuards(t([DOGC]), 0.6, t(filtered), remember, t(daylight), None if spans is None else np.array(spans, np.int32).reshape(-1, 3))


def statuses(results, guards, flt=None, ext=None):
    """results: [(window, class, confidence)] of recording 0 -> {(class, first_window): status}, by both forms of the rule."""
    flt = hand_filter() if flt is None else flt
    rows = np.zeros(len(results), host.DETECTION)
    for i, (w, c, x) in enumerate(sorted(results, key=lambda t: t[0])):
        rows[i] = (0, w, c, x)
    one = guardref.events(rows, flt, ext, guards)
    n_win = max(w for w, _, _ in results) + 1
    bank = guardref.EventBank(1, N, K, flt, ext, guards)
    bank.set_daylight(0, [] if guards.daylight_spans is None else [(lo, hi) for _, lo, hi in guards.daylight_spans.tolist()])
    got = []
    for w in range(n_win):
        here = [(c, x) for ww, c, x in results if ww == w]
        assert len(here) <= K
        conf, idx = np.zeros((1, K), np.float32), np.full((1, K), -1, np.int32)
        for i, (c, x) in enumerate(here):
            conf[0, i], idx[0, i] = x, c
        got.append(bank.process([0], conf, idx))
    got.append(bank.flush())
    assert np.array_equal(by_key(got), one)
    return {(int(e["class_index"]), int(e["first_window"])): int(e["status"]) for e in one}


def test_remember_is_measured_from_the_deadline():
    # the bird opens at 10: d = 13
    assert statuses([(9, DOGC, 0.7), (10, BIRD, 0.9)], hand_guards(remember=4)) == {(BIRD, 10): DOG}          # d - v = 4 == remember: dropped
    assert statuses([(8, DOGC, 0.7), (10, BIRD, 0.9)], hand_guards(remember=4)) == {(BIRD, 10): KEPT}         # d - v = 5 == remember + 1: kept
    assert statuses([(12, DOGC, 0.7), (10, BIRD, 0.9)], hand_guards(remember=1)) == {(BIRD, 10): DOG}         # v == d - 1 counts
    assert statuses([(13, DOGC, 0.7), (10, BIRD, 0.9)], hand_guards(remember=9)) == {(BIRD, 10): KEPT}        # v == d does not
    assert statuses([(20, DOGC, 0.7), (10, BIRD, 0.9)], hand_guards(remember=99)) == {(BIRD, 10): KEPT}       # ... nor any later bark
    assert statuses([(2, DOGC, 0.7), (10, BIRD, 0.9)], hand_guards(remember=11)) == {(BIRD, 10): DOG}         # a bark long before b counts
    assert statuses([(10, BIRD, 0.9), (10, OWL, 0.9)], hand_guards(remember=99)) == {(BIRD, 10): KEPT, (OWL, 10): KEPT}      # no bark: nothing dropped
    assert statuses([(9, DOGC, 0.7), (10, OWL, 0.9)], hand_guards(remember=99)) == {(OWL, 10): KEPT}          # a species not in the list
    assert statuses([(9, DOGC, 0.6), (10, BIRD, 0.9)], hand_guards(remember=99)) == {(BIRD, 10): KEPT}        # x == dog_threshold: strict, no hit
    assert statuses([(9, DOGC, np.nan), (10, BIRD, 0.9)], hand_guards(remember=99)) == {(BIRD, 10): KEPT}
    assert statuses([(9, DOGC, 0.7), (10, BIRD, 0.9)], hand_guards(remember=0)) == {(BIRD, 10): KEPT}         # remember 0 reaches no window before d


def test_only_the_latest_bark_before_the_deadline_matters():
    # barks at 2 and 12, d = 13: the later one decides; a bark at 14 lies behind d and is not looked at
    assert statuses([(2, DOGC, 0.7), (12, DOGC, 0.7), (14, DOGC, 0.7), (10, BIRD, 0.9)], hand_guards(remember=1)) == {(BIRD, 10): DOG}
    # the next event of the same species, d = 33: the latest bark before it is 14, out of reach
    got = statuses([(12, DOGC, 0.7), (14, DOGC, 0.7), (10, BIRD, 0.9), (30, BIRD, 0.9)], hand_guards(remember=3))
    assert got == {(BIRD, 10): DOG, (BIRD, 30): KEPT}


def test_sliding_deadline_is_the_one_measured_from():
    x = extend(None, max_windows=14, short_wait=2, medium_from=5, medium_wait=4, long_from=9, long_wait=6)
    # hits at 10, 12: d = min(12 + max(3, 2), 24) = 15; the bark at 14 lies before it, and d - v = 1
    assert statuses([(10, BIRD, 0.9), (12, BIRD, 0.9), (14, DOGC, 0.7)], hand_guards(remember=1), ext=x) == {(BIRD, 10): DOG}
    assert statuses([(10, BIRD, 0.9), (14, DOGC, 0.7)], hand_guards(remember=1), ext=x) == {(BIRD, 10): KEPT}    # d = 13: the bark is behind it


def test_daylight_edges():
    g = hand_guards(spans=[(0, 10, 20)])
    assert statuses([(10, OWL, 0.9)], g) == {(OWL, 10): DAYLIGHT}                                             # b == from: dropped
    assert statuses([(19, OWL, 0.9)], g) == {(OWL, 19): DAYLIGHT}
    assert statuses([(20, OWL, 0.9)], g) == {(OWL, 20): KEPT}                                                 # b == to: kept
    assert statuses([(9, OWL, 0.9), (10, OWL, 0.9)], g) == {(OWL, 9): KEPT}                                   # FirstDetected decides, not the later hits
    assert statuses([(10, BIRD, 0.9)], g) == {(BIRD, 10): KEPT}                                               # a species not in the list
    assert statuses([(10, OWL, 0.9)], hand_guards(spans=None)) == {(OWL, 10): KEPT}                           # no span: fails open
    two = hand_guards(spans=[(0, 2, 4), (0, 10, 20)])
    assert statuses([(4, OWL, 0.9), (12, OWL, 0.9)], two) == {(OWL, 4): KEPT, (OWL, 12): DAYLIGHT}


def test_the_first_test_that_applies_is_the_status():
    both = hand_guards(remember=9, spans=[(0, 0, 50)], filtered=(BIRD,), daylight=(BIRD,))
    few = hand_filter(min_count=2)
    assert statuses([(9, DOGC, 0.7), (10, BIRD, 0.9)], both, flt=few) == {(BIRD, 10): FEW}                    # few and dog: 1
    assert statuses([(10, BIRD, 0.9), (11, BIRD, 0.9), (11, HUMAN, 0.9)], both, flt=few) == {(BIRD, 10): VETOED}      # vetoed and daylight: 2
    assert statuses([(9, DOGC, 0.7), (10, BIRD, 0.9), (11, BIRD, 0.9)], both, flt=few) == {(BIRD, 10): DOG}   # dog and daylight: 3
    assert statuses([(10, BIRD, 0.9), (11, BIRD, 0.9)], both, flt=few) == {(BIRD, 10): DAYLIGHT}
    # without KEEP_DROPPED none of them is answered
    assert statuses([(9, DOGC, 0.7), (10, BIRD, 0.9), (11, BIRD, 0.9)], both, flt=hand_filter(2, 0)) == {}


def test_a_dog_class_is_a_class_like_any_other():
    g = hand_guards(remember=9, filtered=(BIRD, DOGC))
    # 0.7 marks and stays below the dog's own species threshold 0.8: no dog event; 0.9 marks and forms one - which its own bark drops
    assert statuses([(9, DOGC, 0.7), (10, BIRD, 0.9)], g) == {(BIRD, 10): DOG}
    assert statuses([(9, DOGC, 0.9), (10, BIRD, 0.9)], g) == {(DOGC, 9): DOG, (BIRD, 10): DOG}
    assert statuses([(9, DOGC, 0.9), (10, BIRD, 0.9)], hand_guards(remember=9)) == {(DOGC, 9): KEPT, (BIRD, 10): DOG}
    # a dog class that is also a veto class marks and forms no event
    t = lambda cs: np.isin(np.arange(N), cs).astype(np.uint8)
    g = host.EventGuards(t([HUMAN]), 0.6, t([BIRD]), 9, None, None)
    assert statuses([(5, HUMAN, 0.9), (10, BIRD, 0.9)], g) == {(BIRD, 10): DOG}


def test_restatement_bank_settings():
    """Dog windows are recorded only under guards with a dog table, survive flush and set_guards(None), and go with a reset; a failed
    call leaves them alone; spans are a setting read at the flush."""
    flt = hand_filter()
    g = hand_guards(remember=50, spans=None)
    row = lambda *res: (np.array([[x for _, x in res] + [0.0] * (K - len(res))], np.float32),
                        np.array([[c for c, _ in res] + [-1] * (K - len(res))], np.int32))
    bank = guardref.EventBank(2, N, K, flt, None, None)
    bank.process([0], *row((DOGC, 0.7)))                                 # window 0: no guards, not recorded
    bank.set_guards(g)
    bank.process([0], *row((BIRD, 0.9)))                                 # window 1
    assert [int(e["status"]) for e in bank.flush()] == [KEPT]
    bank.process([0], *row((DOGC, 0.7), (BIRD, 0.9)))                    # window 2: recorded
    with pytest.raises(guardref.TooSmall):
        bank.process([0, 0, 0], *[np.concatenate(a) for a in zip(row((DOGC, 0.7)), row(), row())], cap=0)
    assert bank.src[0].dog == 2 and bank.clock(0) == 3
    assert [int(e["status"]) for e in bank.flush()] == [DOG]
    bank.set_guards(None)
    bank.process([0], *row((DOGC, 0.7)))                                 # window 3: not recorded
    bank.set_guards(g)
    bank.process([0, 1], *[np.concatenate(a) for a in zip(row((BIRD, 0.9)), row((BIRD, 0.9)))])
    assert bank.src[0].dog == 2
    assert [(int(e["recording"]), int(e["status"])) for e in bank.flush()] == [(0, DOG), (1, KEPT)]          # per source
    bank.reset(0)
    bank.process([0], *row((BIRD, 0.9)))
    assert [int(e["status"]) for e in bank.flush()] == [KEPT]
    # daylight: read at the flush
    bank.set_daylight(0, [(0, 5)])
    bank.process([0], *row((OWL, 0.9)))                                  # window 1 of source 0
    bank.set_daylight(0, [])
    assert [int(e["status"]) for e in bank.flush()] == [KEPT]
    bank.process([0], *row((OWL, 0.9)))
    bank.set_daylight(0, [(0, 5)])
    assert [int(e["status"]) for e in bank.flush()] == [DAYLIGHT]
    bank.reset(0)
    assert bank.day.get(0, []) == []
    with pytest.raises(ValueError):
        bank.set_daylight(0, [(i, i + 1) for i in range(0, 18, 2)])
    with pytest.raises(ValueError):
        bank.set_daylight(-1, [(0, 1)])


# ------------------------------------------------------------------------------------------ the library, no device
def test_symbols_and_refusals(built_lib):
    lib = host._analyze_clips_protos(host._event_bank_protos(host.load_library()))
    for name in ("bnhip_detection_events_guarded", "bnhip_analyze_channels_pcm_events_guarded", "bnhip_analyze_channels_pcm_clips_guarded",
                 "bnhip_event_bank_set_guards", "bnhip_event_bank_set_daylight"):
        assert name in host.SYMBOLS and getattr(lib, name) is not None, name
    assert (host.EVENT_DOG, host.EVENT_DAYLIGHT, host.EVENT_DAYLIGHT_SPANS) == (DOG, DAYLIGHT, guardref.DAYLIGHT_SPANS) == (3, 4, 8)
    thr = np.full(8, 0.5, np.float32)
    fs = host._EventFilterStruct(thr.ctypes.data, None, 0.5, 5, 1, 0)
    n, ev = C.c_size_t(777), np.zeros(2, host.EVENT)
    good = dict(max_windows=20, short_wait=2, medium_from=5, medium_wait=4, long_from=9, long_wait=6)
    xs = extend(None, **good)._struct(8)

    def entry(spans=None, n_spans=None, remember=0, null=False, px=None, filt=fs):
        sp = None if spans is None else np.array(spans, np.int32).reshape(-1, 3)
        gs = host._EventGuardsStruct(None, None, None, None if sp is None else sp.ctypes.data, 0.5, remember,
                                     (0 if sp is None else sp.shape[0]) if n_spans is None else n_spans, 0)
        ev[:] = 0
        rc = lib.bnhip_detection_events_guarded(0, None, 0, 8, None if filt is None else C.addressof(filt), px, None if null else C.addressof(gs),
                                                ev.ctypes.data, 2, C.byref(n))
        assert not ev.view(np.uint8).any()
        return rc

    for kw, text in [(dict(null=True), b"NULL event guards"), (dict(remember=-1), b"dog_remember_windows must not be negative"),
                     (dict(n_spans=-1), b"n_spans must be in [0, 2^20]"), (dict(spans=[(0, 0, 1)], n_spans=(1 << 20) + 1), b"n_spans must be in [0, 2^20]"),
                     (dict(n_spans=1), b"NULL daylight_spans"),
                     (dict(spans=[(0, 5, 9), (0, 2, 4)]), b"ascend"), (dict(spans=[(1, 0, 4), (0, 5, 9)]), b"ascend"),
                     (dict(spans=[(0, 2, 6), (0, 5, 9)]), b"not overlap"), (dict(spans=[(0, 4, 4)]), b"0 <= from < to"),
                     (dict(spans=[(0, 6, 4)]), b"0 <= from < to"), (dict(spans=[(0, -1, 4)]), b"0 <= from < to"),
                     (dict(spans=[(-1, 1, 4)]), b"recording outside the call"), (dict(spans=[(65535, 1, 4)]), b"recording outside the call"),
                     (dict(filt=None), b"NULL event filter")]:
        n.value = 777
        assert entry(**kw) == host.E_INVALID and text in lib.bnhip_last_error(), (kw, lib.bnhip_last_error())
        assert n.value == 777
    # the extend may be NULL; one that is given is checked as the _extended entry checks it
    bad = extend(None, **dict(good, max_windows=4))._struct(8)
    assert entry(px=C.addressof(bad)) == host.E_INVALID and b"max_windows must be at least hold_windows" in lib.bnhip_last_error()
    for px in (None, C.addressof(xs)):
        n.value = 777
        assert entry(px=px, spans=[(0, 2, 4), (0, 4, 9), (65534, 0, 1)]) == host.BNHIP_OK and n.value == 0     # (no rows: no device)
    # the entries that need a handle refuse a NULL one
    assert lib.bnhip_event_bank_set_guards(None, None) == host.E_INVALID and b"NULL" in lib.bnhip_last_error()
    assert lib.bnhip_event_bank_set_daylight(None, 0, None, 0) == host.E_INVALID and b"NULL" in lib.bnhip_last_error()
    # the Python layer: a table of another size
    with pytest.raises(host.HipError, match="n_classes"):
        host.detection_events(np.zeros(0, host.DETECTION), 8, host.EventTables(thr, None, 0.5, 5, 1, 0),
                              guards=host.EventGuards(np.zeros(7, np.uint8)))


# ------------------------------------------------------------------------------------------ the Python layers
def test_dog_labels_by_the_reference_rule():
    from birdnet_go_amd import wav
    for label in ("Dog_Dog", "Dog_Hund", "dog_perro", "Dog", "BARK", "Growling", "Canis familiaris"):
        assert wav.is_dog_label(label), label
    for label in ("Poecilimon doga_Poecilimon doga", "Canis lupus", "Canis latrans_Coyote", "Howl", "Hot dog", "Human vocal_Human vocal"):
        assert not wav.is_dog_label(label), label


def test_wav_event_guards_tables():
    from birdnet_go_amd import wav
    labels = ["Dog_Hund", "Strix aluco_Tawny Owl", "Turdus merula_Blackbird", "Poecilimon doga_Katydid", "Bark"]
    g = wav.EventGuards(0.1, species=["Turdus merula_Blackbird", 3], remember_minutes=0.05, daylight_species=[1],
                        daylight={"a.wav": [(0.0, 2.5), (4.0, 4.1), (7.2, 7.9)], "c.wav": [(1.5, 3.0)]})
    t = g.tables(5, 48000, 48000, labels, ["b.wav", "a.wav", "c.wav"])          # windows of 1 s
    assert t.class_dog.tolist() == [1, 0, 0, 0, 1] and t.class_dog_filtered.tolist() == [0, 0, 1, 1, 0] and t.class_daylight.tolist() == [0, 1, 0, 0, 0]
    # a window is in daylight when it begins in [from, to): both edges up to the next window start; (7.2, 7.9) holds none
    assert t.daylight_spans.tolist() == [[1, 0, 3], [1, 4, 5], [2, 2, 3]]
    assert t.dog_remember_windows == 3 and np.float32(t.dog_threshold) <= np.float32(0.1)
    assert wav.EventGuards(0.1, remember_minutes=1.0).tables(5, 48000, 72000, labels).dog_remember_windows == 40
    none = wav.EventGuards(0.5, dog_labels=[]).tables(5, 48000, 48000, labels)
    assert none.class_dog is None and none.class_dog_filtered is None and none.class_daylight is None and none.daylight_spans is None
    assert wav.EventGuards(0.5, dog_labels=[2]).tables(5, 48000, 48000, labels).class_dog.tolist() == [0, 0, 1, 0, 0]
    with pytest.raises(ValueError):
        wav.EventGuards(0.1, species=["no such bird"]).tables(5, 48000, 48000, labels)
    with pytest.raises(ValueError):
        wav.EventGuards(0.1, daylight={"a.wav": [(5.0, 9.0), (2.0, 3.0)]}).tables(5, 48000, 48000, labels, ["a.wav"])
    with pytest.raises(ValueError):
        wav.EventGuards(0.1, remember_minutes=-1.0)
    with pytest.raises(ValueError, match="guards need events"):
        wav.analyze_files(["a.wav"], None, guards=g)


def test_window_batcher_refuses_guards_it_would_ignore():
    from birdnet_go_amd import stream as S
    flt = host.EventTables(np.full(8, 0.5, np.float32), None, 0.5, 5, 1, 0)
    for kw in (dict(events=None), dict(events=flt, native=False)):
        with pytest.raises(S.StreamError, match="guards need events and the native rings"):
            S.WindowBatcher(S.Orchestrator(), guards=host.EventGuards(), **kw)
        wb = S.WindowBatcher(S.Orchestrator(), **kw)
        with pytest.raises(S.StreamError, match="guards need events and the native rings"):
            wb.set_guards(None)
        with pytest.raises(S.StreamError, match="guards need events and the native rings"):
            wb.set_daylight("mic", [(0.0, 1.0)])
