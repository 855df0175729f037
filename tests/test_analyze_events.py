"""Detection events on the device: bnhip_detection_events over crafted rows, and the fused bnhip_analyze_*_pcm_events entries with the
tiny FFT model and the five-recording burst of tests/test_analyze.py.

Every comparison is np.array_equal against the restatement of the rule (tests/evref.py): the rule has compares and a maximum, no
arithmetic, so there is no tolerance to choose.  Each crafted case runs with and without BNHIP_EVENTS_KEEP_DROPPED."""
import numpy as np
import pytest

from birdnet_go_amd import host, wav

import evref
from test_analyze import CLIP, HOP, K, LENGTHS, MIN_TAIL, _bytes, _fft_tiny_blob, _recordings, _write_wav16

pytestmark = pytest.mark.gpu


def _rows(items):
    """[(recording, window, class, confidence), ...] as given -> DETECTION."""
    rows = np.zeros(len(items), host.DETECTION)
    for i, q in enumerate(items):
        rows[i] = q
    return rows


def _flt(thr, veto=None, veto_threshold=0.5, hold=4, min_count=1, flags=0):
    return host.EventTables(np.asarray(thr, np.float32), veto, veto_threshold, hold, min_count, flags)


def _both(rows, n_classes, **kw):
    """The device tail against the restatement, dropped events left out and kept; -> the events with their statuses."""
    for flags in (0, host.EVENTS_KEEP_DROPPED):
        f = _flt(flags=flags, **kw)
        got, want = host.detection_events(rows, n_classes, f), evref.events(rows, f)
        assert got.dtype == evref.EVENT and np.array_equal(got, want), (flags, got, want)
    return got


def _fields(ev, *names):
    return [tuple(int(e[n]) for n in names) for e in ev]


# ------------------------------------------------------------------------------------------ crafted rows, no model
def test_no_rows_and_one_row(gpu):
    assert _both(np.zeros(0, host.DETECTION), 3, thr=[0.5] * 3).size == 0
    one = _both(_rows([(2, 9, 1, 0.75)]), 3, thr=[0.5] * 3)
    assert one.tolist() == [(2, 1, 9, 9, 9, 1, 0.75, 0)]
    assert _both(_rows([(2, 9, 1, 0.25)]), 3, thr=[0.5] * 3).size == 0


@pytest.mark.parametrize("n", [255, 256, 257, 1025])
def test_block_boundaries(gpu, n):
    """One recording, a row per window, the classes in turn: every (recording, class) group runs through the whole input and
    straddles row 256 (and, sorted, the groups' borders fall inside blocks)."""
    rng = np.random.default_rng(n)
    rows = np.zeros(n, host.DETECTION)
    rows["window"], rows["class_index"] = np.arange(n), np.arange(n) % 3
    rows["confidence"] = (rng.integers(0, 32, n) / 32.0).astype(np.float32)
    ev = _both(rows, 5, thr=[0.25, 0.5, 0.0, 0.0, 0.0], hold=4, min_count=2)
    assert ev.size > n // 16 and set(ev["status"]) == {0, 1}


def test_keys_at_both_ends(gpu):
    """Recording 0 class 0 and recording 65 534 class 38 399 of 38 400: the largest key there is, so the fourth radix pass runs."""
    nc = 38400
    rows = _rows([(0, 0, 0, 0.9), (0, 1, nc - 1, 0.8), (0, 2, 0, 0.95), (1, 0, 255, 0.9), (1, 0, 256, 0.9), (65534, 3, 0, 0.7), (65534, 4, nc - 1, 0.9),
                  (65534, 5, nc - 1, 0.6)])
    thr = np.full(nc, 0.5, np.float32)
    ev = _both(rows, nc, thr=thr)
    assert _fields(ev, "recording", "class_index", "count") == [(0, 0, 2), (0, nc - 1, 1), (1, 255, 1), (1, 256, 1), (65534, 0, 1), (65534, nc - 1, 2)]


def test_hold_boundaries(gpu):
    ev = _both(_rows([(0, 0, 1, 0.6), (0, 3, 1, 0.7), (0, 4, 1, 0.8)]), 2, thr=[0.5, 0.5], hold=4)
    assert _fields(ev, "first_window", "last_window", "count") == [(0, 3, 2), (4, 4, 1)]
    assert ev["confidence"].tolist() == [np.float32(0.7), np.float32(0.8)] and ev["best_window"].tolist() == [3, 4]


def test_greedy_restart(gpu):
    """A hit in every window 0..20 at hold 4: the hold counts from an event's first hit, so six events - not one merged by its gaps."""
    ev = _both(_rows([(0, w, 0, 0.9) for w in range(21)]), 1, thr=[0.5], hold=4)
    assert _fields(ev, "first_window", "last_window", "count") == [(0, 3, 4), (4, 7, 4), (8, 11, 4), (12, 15, 4), (16, 19, 4), (20, 20, 1)]


@pytest.mark.parametrize("hold", [1, 7, 100000])
def test_skew(gpu, hold):
    """One class hits in 3 000 consecutive windows of a recording, beside 200 groups of one hit: the walk of the long group passes
    through many 64-hit steps and across the blocks, whatever lies around it."""
    items = [(0, w, 5, 0.6 + 0.3 * ((w * 7) % 11) / 11.0) for w in range(3000)] + [(0, 10 * j, 6 + j, 0.9) for j in range(200)]
    items += [(1, w, 5, 0.9) for w in range(70)]
    rows = _rows(items)
    rows = rows[np.lexsort((rows["window"], rows["recording"]))]
    ev = _both(rows, 256, thr=[0.5] * 256, hold=hold, min_count=1)
    long = ev[(ev["recording"] == 0) & (ev["class_index"] == 5)]
    assert long.size == -(-3000 // hold) and int(long["count"].sum()) == 3000 and ev.size == long.size + 200 + -(-70 // hold)


def test_equal_confidences_keep_the_earliest(gpu):
    ev = _both(_rows([(0, 2, 0, 0.5), (0, 3, 0, 0.75), (0, 4, 0, 0.75), (0, 5, 0, 0.5)]), 1, thr=[0.25], hold=10)
    assert _fields(ev, "first_window", "last_window", "best_window", "count") == [(2, 5, 3, 4)]


def test_what_is_a_hit(gpu):
    """x == threshold and a NaN confidence are dropped; thresholds +inf and NaN exclude their classes; a row given twice counts twice."""
    nan, inf = float("nan"), float("inf")
    rows = _rows([(0, 0, 0, 0.5), (0, 0, 1, nan), (0, 0, 2, 1.0), (0, 0, 3, 1.0), (0, 1, 4, 0.625), (0, 1, 4, 0.625), (0, 2, 0, np.nextafter(np.float32(0.5), np.float32(1))),
                  (0, 2, 2, inf)])
    ev = _both(rows, 5, thr=[0.5, 0.0, inf, nan, 0.5], hold=1)
    assert _fields(ev, "class_index", "first_window", "count") == [(0, 2, 1), (4, 1, 2)]


def test_veto(gpu):
    """Hold 4, events of class 0 at b = 10 in recordings 0..5; class 1 is the veto class, heard at another window in each."""
    veto = np.array([0, 1, 0], np.uint8)
    items = []
    for r, v, x in [(0, 10, 0.9), (1, 13, 0.9), (2, 9, 0.9), (3, 14, 0.9), (4, 12, 0.5), (5, None, 0.0)]:
        items += [(r, 10, 0, 0.8), (r, 11, 0, 0.7)]
        if v is not None:
            items.append((r, v, 1, x))
    items += [(6, 11, 1, 0.9)]                                          # heard in another recording: no effect on recording 5
    rows = _rows(items)
    rows = rows[np.lexsort((rows["window"], rows["recording"]))]
    ev = _both(rows, 3, thr=[0.5, 0.0, 0.5], veto=veto, veto_threshold=0.5, hold=4)
    # at b and at b + hold - 1: vetoed; at b - 1 and at b + hold: not; x == veto_threshold: not a veto; the veto class, for all its low
    # class_threshold, forms no event
    assert _fields(ev, "recording", "class_index", "status") == [(0, 0, 2), (1, 0, 2), (2, 0, 0), (3, 0, 0), (4, 0, 0), (5, 0, 0)]


def test_min_count_and_the_order_of_the_tests(gpu):
    veto = np.array([0, 1], np.uint8)
    rows = _rows([(0, 0, 0, 0.9), (0, 1, 0, 0.9), (0, 2, 0, 0.9),       # count == min_count: kept
                  (0, 20, 0, 0.9), (0, 21, 0, 0.9),                     # count == min_count - 1: status 1
                  (1, 0, 0, 0.9), (1, 0, 1, 0.9), (1, 1, 0, 0.9),       # short AND vetoed: status 1, decided first
                  (2, 0, 0, 0.9), (2, 1, 0, 0.9), (2, 1, 1, 0.9), (2, 2, 0, 0.9)])   # enough hits, vetoed: status 2
    ev = _both(rows, 2, thr=[0.5, 0.5], veto=veto, veto_threshold=0.5, hold=4, min_count=3)
    assert _fields(ev, "recording", "first_window", "count", "status") == [(0, 0, 3, 0), (0, 20, 2, 1), (1, 0, 2, 1), (2, 0, 3, 2)]
    kept = host.detection_events(rows, 2, _flt([0.5, 0.5], veto, 0.5, 4, 3, 0))
    assert _fields(kept, "recording", "first_window", "status") == [(0, 0, 0)]


def _sweep_rows(seed=5, n=20000, n_rec=7, n_classes=50, n_windows=400):
    rng = np.random.default_rng(seed)
    rows = np.zeros(n, host.DETECTION)
    rows["recording"], rows["window"] = rng.integers(0, n_rec, n), rng.integers(0, n_windows, n)
    rows["class_index"] = rng.integers(0, n_classes, n)
    rows["confidence"] = (rng.integers(0, 64, n) / 64.0).astype(np.float32)
    rows["confidence"][rng.integers(0, n, 200)] = np.nan
    return rows[np.lexsort((rows["window"], rows["recording"]))]


def test_cap_below_the_total(gpu):
    rows = _sweep_rows(n=3000)
    f = _flt(np.full(50, 0.5, np.float32), hold=3, flags=host.EVENTS_KEEP_DROPPED)
    want = evref.events(rows, f)
    for cap in (0, 1, 257, want.size, want.size + 5):
        got, total = host.detection_events(rows, 50, f, cap=cap)
        assert total == want.size and np.array_equal(got, want[:cap])


def test_sweep_twice_the_same_bytes(gpu):
    rows = _sweep_rows()
    rng = np.random.default_rng(6)
    thr = (rng.integers(8, 56, 50) / 64.0).astype(np.float32)
    thr[11], thr[12] = np.inf, np.nan
    veto = np.zeros(50, np.uint8)
    veto[[3, 30]] = 1
    f = _flt(thr, veto, 0.9, hold=5, min_count=2, flags=host.EVENTS_KEEP_DROPPED)
    want = evref.events(rows, f)
    assert set(want["status"]) == {0, 1, 2}
    a, b = host.detection_events(rows, 50, f), host.detection_events(rows, 50, f)
    assert np.array_equal(a, want) and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------ the fused entries
def _between(values, q):
    """A threshold between two neighbouring observed confidences, near quantile q of the distinct values."""
    v = np.unique(values)
    if v.size < 2:
        return np.float32(v[0])
    i = min(max(int(q * (v.size - 1)), 0), v.size - 2)
    return np.float32((float(v[i]) + float(v[i + 1])) / 2)


def _pick_filter(rows, n_classes, need=(0, 1, 2)):
    """Thresholds from the observed rows - per class a value between its confidences - and one veto class, such that the RESTATEMENT
    finds an event of every status in `need`: a property of the inputs, searched here without the code under test."""
    for q in (0.5, 0.35, 0.65, 0.2, 0.8):
        thr = np.full(n_classes, np.inf, np.float32)
        for c in np.unique(rows["class_index"]):
            thr[c] = _between(rows["confidence"][rows["class_index"] == c], q)
        for hold in (3, 2, 5):
            for min_count in (2, 3):
                for vc in np.unique(rows["class_index"]):
                    veto = np.zeros(n_classes, np.uint8)
                    veto[vc] = 1
                    for vq in (0.5, 0.8, 0.2):
                        f = _flt(thr, veto, float(_between(rows["confidence"][rows["class_index"] == vc], vq)), hold, min_count,
                                 host.EVENTS_KEEP_DROPPED)
                        if set(need) <= set(evref.events(rows, f)["status"]):
                            return f
    raise AssertionError("the rows give no filter with an event of every status")


def _without_dropped(f):
    return host.EventTables(f.class_threshold, f.class_veto, f.veto_threshold, f.hold_windows, f.min_count, 0)


@pytest.fixture(scope="module")
def clf(gpu):
    c = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False)
    yield c
    c.close()


def test_fused_burst(clf):
    """The five-recording burst with its last recording lengthened to just over 2^20 samples (190 windows: six chunks at max_batch
    32), so that the slot block alone is past the 2 MiB from which a call's device parts share one block (DEV_OWN_BLOCK,
    csrc/api_oneshot.h) while every table beside it is far below.  The existing entries answer the same bytes before and after the
    events calls on the same handle."""
    lengths = LENGTHS[:-1] + [175 * HOP + 2]                                # (as the burst's own last recording: a tail that is dropped)
    assert lengths[-1] > 1 << 20 and host.analyze_windows(lengths, CLIP, HOP, MIN_TAIL)[-1] == 190
    recs = _recordings(lengths)
    raw, n_classes = _bytes(np.concatenate(recs), 16), clf.num_species()
    rows, total = clf.analyze_pcm(raw, 16, lengths, HOP, MIN_TAIL, k=K, threshold=0.0)
    topk = clf.analyze_pcm_topk(raw, 16, lengths, HOP, MIN_TAIL, k=K)
    assert total == rows.size == 190 * K
    f = _pick_filter(rows, n_classes)
    want = evref.events(rows, f)
    assert set(want["status"]) == {0, 1, 2}                              # the comparison cannot pass empty
    got = clf.analyze_pcm_events(raw, 16, lengths, HOP, f, MIN_TAIL, k=K)
    assert np.array_equal(got, want)
    kept = clf.analyze_pcm_events(raw, 16, lengths, HOP, _without_dropped(f), MIN_TAIL, k=K)
    assert kept.size and np.array_equal(kept, want[want["status"] == 0])
    few, n = clf.analyze_pcm_events(raw, 16, lengths, HOP, f, MIN_TAIL, k=K, cap=2)
    assert n == want.size and np.array_equal(few, want[:2])
    assert np.array_equal(host.detection_events(rows, n_classes, f), want)       # the tail alone, over the rows brought down
    again, total2 = clf.analyze_pcm(raw, 16, lengths, HOP, MIN_TAIL, k=K, threshold=0.0)
    topk2 = clf.analyze_pcm_topk(raw, 16, lengths, HOP, MIN_TAIL, k=K)
    assert total2 == total and again.tobytes() == rows.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(topk, topk2))


def test_fused_mixed(clf):
    """Two recordings at two rates and depths: the resampling route of the mixed call, then the same tail."""
    a, b = _recordings([9 * CLIP + 3, 6 * CLIP + 1], seed=21)
    raw = _bytes(a, 16) + _bytes(b, 24)
    recs = host.recordings([a.size, b.size], [48000, 32000], [16, 24])
    rows, _ = clf.analyze_mixed_pcm(raw, recs, 48000, HOP, MIN_TAIL, k=K, threshold=0.0)
    assert set(rows["recording"]) == {0, 1}
    f = _pick_filter(rows, clf.num_species(), need=(0, 1))
    want = evref.events(rows, f)
    assert want.size and np.array_equal(clf.analyze_mixed_pcm_events(raw, recs, 48000, HOP, f, MIN_TAIL, k=K), want)
    # a burst at the model's rate and one depth takes the plain body
    plain = host.recordings([a.size], 48000, 16)
    rows1, _ = clf.analyze_pcm(_bytes(a, 16), 16, [a.size], HOP, MIN_TAIL, k=K, threshold=0.0)
    assert np.array_equal(clf.analyze_mixed_pcm_events(_bytes(a, 16), plain, 48000, HOP, f, MIN_TAIL, k=K), evref.events(rows1, f))


def test_fused_channels(clf):
    """One stereo recording, the channel left to the device: the events of the rows of the _pcm entry, and the same choice."""
    left, right = _recordings([9 * CLIP + 3, 9 * CLIP + 3], seed=31)
    frames = np.stack([left, (right // 64).astype(np.int16)], axis=1).reshape(-1)          # the left channel leads by far more than 6 dB
    raw = _bytes(frames, 16)
    recs = host.channel_recordings([left.size], 48000, 16, 2, "auto")
    rows, _, chosen = clf.analyze_channels_pcm(raw, recs, 48000, HOP, MIN_TAIL, k=K, threshold=0.0)
    f = _pick_filter(rows, clf.num_species(), need=(0, 1))
    want = evref.events(rows, f)
    got, chosen_ev = clf.analyze_channels_pcm_events(raw, recs, 48000, HOP, f, MIN_TAIL, k=K)
    assert want.size and np.array_equal(got, want) and chosen_ev.tolist() == chosen.tolist() == [0]


def test_analyze_files_events(clf, tmp_path):
    """wav.analyze_files(events=...) on every route answers the tuples computed from the events of the restatement."""
    recs = _recordings(LENGTHS)
    paths = []
    for i, x in enumerate(recs):
        paths.append(str(tmp_path / f"r{i}.wav"))
        _write_wav16(paths[-1], x)
    rate, n_classes = 48000, clf.num_species()
    clip_seconds, overlap = CLIP / rate, (CLIP - HOP) / rate
    clip_len, hop, min_tail = wav._framing(rate, clip_seconds, overlap, 1.0)
    assert (clip_len, hop) == (CLIP, HOP)
    rows, _ = clf.analyze_pcm(_bytes(np.concatenate(recs), 16), 16, LENGTHS, hop, min_tail, k=K, threshold=0.0)
    f = _pick_filter(rows, n_classes)
    finite = np.isfinite(f.class_threshold)
    flt = wav.EventFilter(default_threshold=np.inf, thresholds={int(c): float(f.class_threshold[c]) for c in np.flatnonzero(finite)},
                          veto=np.flatnonzero(f.class_veto).tolist(), veto_threshold=f.veto_threshold, hold_seconds=f.hold_windows * hop / rate,
                          min_count=f.min_count, keep_dropped=True)
    tables = flt.tables(n_classes, rate, hop, overlap)
    assert np.array_equal(tables.class_threshold, f.class_threshold) and tables.hold_windows == f.hold_windows
    want = [[] for _ in paths]
    for e in evref.events(rows, f):
        want[e["recording"]].append((float(np.float64(int(e["first_window"]) * hop) / rate),
                                     float(np.float64(int(e["last_window"]) * hop) / rate + clip_seconds), int(e["class_index"]),
                                     float(e["confidence"]), int(e["count"]), int(e["status"])))
    assert sum(len(w) for w in want) > 0
    kw = dict(overlap_seconds=overlap, top_k=K, model_rate=rate, events=flt)
    assert wav.analyze_files(paths, clf, **kw) == want
    assert wav.analyze_files(paths, clf, device_resample=True, **kw) == want
    got, chosen = wav.analyze_files(paths, clf, channels=0, return_chosen=True, **kw)
    assert got == want and chosen == [0] * len(paths)
    flt.keep_dropped = False
    assert wav.analyze_files(paths, clf, **kw) == [[t[:5] for t in w if t[5] == 0] for w in want]
