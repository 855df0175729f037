"""The dog-bark and daylight filters on the device: the guarded file tail and a bank under guards over crafted rows, every answer
np.array_equal to the restatement (tests/guardref.py) - the rule is compares and integer arithmetic, so there is no tolerance to
choose - and then through the tiny models: the fused tick, the fused analysis entry, the clip export and a dynamic bank."""
import copy
import ctypes as C

import numpy as np
import pytest

from birdnet_go_amd import host

import evref
import evxref
import guardref
from guardref import DAYLIGHT, DOG, KEPT
from test_analyze import CLIP, HOP, K, MIN_TAIL, _bytes, _fft_tiny_blob, _recordings
from test_event_bank import Pair
from test_event_bank_ref import by_key, detection_rows, feed, filters, topk_rows
from test_event_guards_ref import random_guards, spans_of

pytestmark = pytest.mark.gpu

SMALL = dict(max_windows=14, short_wait=2, medium_from=5, medium_wait=4, long_from=9, long_wait=6)
N_CLASSES, TOP = 40, 3


# the classes the crafted streams draw their results from: 9 of the 40, so that a class comes round often enough to reach a minimum
# count - the two veto classes of `filters` (0, 20), its +inf and NaN thresholds (1, 2) and the dog classes of `random_guards` among them
ACTIVE = np.array([0, 20, 1, 2, 5, 7, 3, 9, 33], np.int32)


def stream(rng, n_src, n_win):
    conf, idx = topk_rows(rng, n_src, n_win, ACTIVE.size, TOP)
    return conf, np.where(idx >= 0, ACTIVE[np.maximum(idx, 0)], -1).astype(np.int32)


def guards(rng, n_rec, n_win, **kw):
    """random_guards over the 40 classes, with the stream's ordinary classes shared out by hand: 3 and 5 under the bark, 7 and 9
    under the daylight, 33 under both."""
    g = random_guards(rng, N_CLASSES, n_rec, n_win, n_dog=3, **kw)
    g.class_dog_filtered[[3, 5, 33]], g.class_daylight[[7, 9, 33]] = 1, 1
    g.class_dog_filtered[[7, 9]], g.class_daylight[[3, 5]] = 0, 0
    return g


def sliding(rng):
    table = (rng.random(N_CLASSES) < 0.5).astype(np.uint8)
    return host.EventExtend(table, **SMALL)


class GPair(Pair):
    """A device bank (plain or extended) and the guarded streaming restatement side by side."""

    def __init__(self, max_sources, n_classes, k, flt, ext=None, guards=None):
        self.dev = host.EventBank(n_classes, k, flt, max_sources, extend=ext, guards=guards)
        self.ref = guardref.EventBank(max_sources, n_classes, k, flt, ext, guards)
        self.n_classes, self.flt, self.ext = n_classes, flt, ext
        assert self.dev.slots_per_source == self.ref.slots_per_source
        self.answers = []

    def set_guards(self, guards):
        self.dev.set_guards(guards)
        self.ref.set_guards(guards)

    def set_daylight(self, source, spans=()):
        self.dev.set_daylight(source, spans)
        self.ref.set_daylight(source, spans)


# ------------------------------------------------------------------------------------------ the file tail
@pytest.mark.parametrize("ext", [False, True])
def test_tail_random_rows(gpu, ext):
    """About 700 rows over 3 recordings: three blocks of the marking scans, so the dog list and the two searches cross blocks; several
    spans in two recordings and none in the third; a dog class that is a veto class and one that forms events of its own."""
    rng = np.random.default_rng(7 + ext)
    conf, idx = stream(rng, 3, 100)
    rows = detection_rows(conf, idx)
    assert 2 * 256 < rows.size < 4 * 256
    x = sliding(rng) if ext else None
    g = guards(rng, 3, 100, remember=4)
    assert len(spans_of(g, 0)) + len(spans_of(g, 1)) > 2 and not spans_of(g, 2)
    saw = set()
    for hold, min_count, flags in [(3, 2, evref.KEEP_DROPPED), (3, 2, 0), (2, 1, evref.KEEP_DROPPED), (4, 1, 0)]:
        flt = filters(rng, N_CLASSES, hold, min_count, True, flags)
        want = guardref.events(rows, flt, x, g)
        got = host.detection_events(rows, N_CLASSES, flt, extend=x, guards=g)
        assert got.dtype == evref.EVENT and np.array_equal(got, want), (hold, min_count, flags)
        saw |= set(want["status"].tolist())
        some, total = host.detection_events(rows, N_CLASSES, flt, extend=x, guards=g, cap=5)
        assert total == want.size and np.array_equal(some, want[:5])
        # guards that can drop nothing answer the namesake's bytes
        plain = host.detection_events(rows, N_CLASSES, flt, extend=x)
        zero = np.zeros(N_CLASSES, np.uint8)
        for idle in (host.EventGuards(), host.EventGuards(zero, 0.1, zero, 9, zero, None),
                     host.EventGuards(g.class_dog, 0.1, None, 9, None, g.daylight_spans)):
            assert host.detection_events(rows, N_CLASSES, flt, extend=x, guards=idle).tobytes() == plain.tobytes()
    assert saw == {0, 1, 2, DOG, DAYLIGHT}, saw


def test_tail_hand_edges(gpu):
    """The hand-worked edges of tests/test_event_guards_ref.py, on the device: d - v == remember, v == d - 1, v == d, b == from, b == to."""
    n, hold = 8, 3
    t = lambda cs: np.isin(np.arange(n), cs).astype(np.uint8)
    thr = np.full(n, 0.5, np.float32)
    thr[6] = 0.8
    flt = host.EventTables(thr, t([7]), 0.5, hold, 1, evref.KEEP_DROPPED)

    def status(items, remember, spans=None):
        rows = np.zeros(len(items), host.DETECTION)
        for i, q in enumerate(sorted(items, key=lambda q: (q[0], q[1]))):
            rows[i] = q
        g = host.EventGuards(t([6]), 0.6, t([1]), remember, t([2]), None if spans is None else np.array(spans, np.int32))
        got = host.detection_events(rows, n, flt, guards=g)
        assert np.array_equal(got, guardref.events(rows, flt, None, g))
        return {(int(e["recording"]), int(e["class_index"]), int(e["first_window"])): int(e["status"]) for e in got}

    assert status([(0, 9, 6, 0.7), (0, 10, 1, 0.9)], 4) == {(0, 1, 10): DOG}
    assert status([(0, 8, 6, 0.7), (0, 10, 1, 0.9)], 4) == {(0, 1, 10): KEPT}
    assert status([(0, 12, 6, 0.7), (0, 10, 1, 0.9)], 1) == {(0, 1, 10): DOG}
    assert status([(0, 13, 6, 0.7), (0, 10, 1, 0.9)], 9) == {(0, 1, 10): KEPT}
    # the bark of another recording does not count, in front of it or behind it
    assert status([(0, 9, 6, 0.7), (1, 10, 1, 0.9), (2, 9, 6, 0.7)], 99) == {(1, 1, 10): KEPT}
    assert status([(0, 10, 2, 0.9), (1, 10, 2, 0.9), (1, 20, 2, 0.9), (2, 10, 2, 0.9)], 0, [(1, 10, 20)]) == \
        {(0, 2, 10): KEPT, (1, 2, 10): DAYLIGHT, (1, 2, 20): KEPT, (2, 2, 10): KEPT}


# ------------------------------------------------------------------------------------------ the bank
@pytest.mark.parametrize("ext", [False, True])
@pytest.mark.parametrize("flags", [0, evref.KEEP_DROPPED])
def test_bank_random_calls(gpu, ext, flags):
    """About 30 calls on 4 sources: several windows of one source in a call, skipped rows, flush of one source and of all, pending,
    reset of one source, set_guards and set_daylight mid-stream, and one call with too small a cap that is then repeated with room."""
    rng = np.random.default_rng(50 + 2 * ext + flags)
    n_src, n_win = 4, 40
    conf, idx = stream(rng, n_src, n_win)
    flt = filters(rng, N_CLASSES, 4, 1, True, flags)                     # (min_count 1: answered events in every stretch of the stream)
    g1 = guards(rng, n_src, n_win, remember=4)
    g2 = guards(rng, n_src, n_win, remember=2, dog_threshold=0.5)
    g1.class_daylight[:] = 1                                             # (every species: what the bark leaves, the daylight takes)
    p = GPair(n_src + 1, N_CLASSES, TOP, flt, sliding(rng) if ext else None, g1)
    for s in range(n_src - 1):                                           # (the last source: no daylight until call 22)
        p.set_daylight(s, [(2 + s, 12), (16, 22 + s)])
    at, failed, saw = [0] * n_src, False, set()
    for call in range(30):
        if call == 9:
            p.set_guards(None)
        if call == 12:
            p.set_guards(g2)
            p.set_daylight(0, [(0, 3), (8, 30)])
        if call == 14:
            saw |= set(p.flush(2)["status"].tolist())
        if call == 18:
            p.reset(1)
            at[1] = 0
            assert p.clocks([1]) == [0]
        if call == 22:
            saw |= set(p.flush()["status"].tolist())
            p.set_daylight(-1)
            for s in (0, 3):
                p.set_daylight(s, [(at[s], at[s] + 20)])
        if call % 5 == 4:
            assert (p.pending()["status"] == guardref.PENDING).all()
        take = [(s, int(rng.integers(1, 4))) for s in range(n_src) if rng.random() < 0.7]
        rows = [(s, at[s] + j) for s, n in take for j in range(n) if at[s] + j < n_win]
        rows = [rows[i] for i in np.argsort([w + rng.random() for _, w in rows], kind="stable")]      # sources interleaved, each in order
        src = [s if rng.random() > 0.1 else -1 for s, _ in rows]                                     # (a skipped row is not a window)
        cf = np.array([conf[s, w] for s, w in rows], np.float32).reshape(len(rows), TOP)
        ix = np.array([idx[s, w] for s, w in rows], np.int32).reshape(len(rows), TOP)
        need = copy.deepcopy(p.ref).process(src, cf, ix).size
        if call >= 15 and need and not failed:
            before = p.pending()
            with pytest.raises(guardref.TooSmall):
                p.ref.process(src, cf, ix, cap=need - 1)
            with pytest.raises(host.HipError) as ei:
                p.dev.process(src, cf, ix, cap=need - 1)
            assert ei.value.needed == need and np.array_equal(p.dev.pending(), before)
            failed = True
        saw |= set(p.process(src, cf, ix)["status"].tolist())
        for s in src:
            if s >= 0:
                at[s] += 1
        assert p.clocks(range(n_src)) == at
    saw |= set(p.flush()["status"].tolist())
    assert failed, "no call answered an event after call 15"
    assert p.pending().size == 0
    assert saw >= ({0, 2, DOG, DAYLIGHT} if flags else {0}), saw
    p.close()


@pytest.mark.parametrize("ext", [False, True])
@pytest.mark.parametrize("plan", ["window", "all", "groups"])
def test_bank_fed_then_flushed_is_the_tail(gpu, ext, plan):
    rng = np.random.default_rng(90 + ext)
    n_src, n_win = 3, 40
    conf, idx = stream(rng, n_src, n_win)
    rows = detection_rows(conf, idx)
    x = sliding(rng) if ext else None
    g = guards(rng, n_src, n_win, remember=4)
    for flags in (0, evref.KEEP_DROPPED):
        flt = filters(rng, N_CLASSES, 3, 2, True, flags)
        p = GPair(n_src, N_CLASSES, TOP, flt, x, g)
        for s in range(n_src):
            p.set_daylight(s, spans_of(g, s))
        feed(p, conf, idx, plan, np.random.default_rng(3))
        p.flush()
        assert p.pending().size == 0
        want = host.detection_events(rows, N_CLASSES, flt, extend=x, guards=g)
        assert np.array_equal(want, guardref.events(rows, flt, x, g)) and np.array_equal(by_key(p.answers), want)
        assert not flags or {DOG, DAYLIGHT} <= set(want["status"].tolist())
        p.close()


def test_bank_without_guards_is_the_bank_before(gpu):
    """A bank that never had guards set, and one whose guards were turned off again, answer evxref's bank: the guards change statuses
    only, so the state the second bank carries over is the state of a bank that never had any."""
    rng = np.random.default_rng(5)
    n_src, n_win = 3, 40
    conf, idx = stream(rng, n_src, n_win)
    flt = filters(rng, N_CLASSES, 3, 1, True, evref.KEEP_DROPPED)
    x = sliding(rng)
    g = guards(rng, n_src, n_win, remember=4)
    never, off = host.EventBank(N_CLASSES, TOP, flt, n_src, extend=x), host.EventBank(N_CLASSES, TOP, flt, n_src, extend=x, guards=g)
    for s in range(n_src):
        off.set_daylight(s, spans_of(g, s))
    ref = evxref.EventBank(n_src, N_CLASSES, TOP, flt, x)
    differ = False
    for lo in range(0, n_win, 4):
        if lo == 20:
            off.set_guards(None)
        src = [s for w in range(lo, lo + 4) for s in range(n_src)]
        cf, ix = conf[:, lo:lo + 4].transpose(1, 0, 2).reshape(-1, TOP), idx[:, lo:lo + 4].transpose(1, 0, 2).reshape(-1, TOP)
        want = ref.process(src, cf, ix)
        assert np.array_equal(never.process(src, cf, ix), want)
        got = off.process(src, cf, ix)
        if lo >= 20:
            assert np.array_equal(got, want)
        else:
            differ |= not np.array_equal(got, want)
            assert all(np.array_equal(got[n], want[n]) for n in got.dtype.names if n != "status")
    assert differ                                                        # (of the input: the guards did drop events while they were on)
    want = ref.flush()
    assert np.array_equal(never.flush(), want) and np.array_equal(off.flush(), want)
    never.close()
    off.close()


def test_bank_refusals(gpu):
    n, k = 8, 2
    flt = host.EventTables(np.full(n, 0.5, np.float32), None, 0.5, 3, 1, 0)
    bank = host.EventBank(n, k, flt, 2, guards=host.EventGuards(None, 0.5, None, 3, np.ones(n, np.uint8)))
    bank.set_daylight(0, [(0, 9)])
    bank.process([0], np.full((1, k), 0.75, np.float32), np.array([[1, 2]], np.int32))
    before = bank.pending()
    assert before.size == 2
    lib = bank._lib
    for source, spans, text in [(0, [(i, i + 1) for i in range(0, 18, 2)], b"0 to 8 daylight spans"), (0, [(5, 9), (2, 4)], b"ascend"),
                                (0, [(2, 6), (5, 9)], b"not overlap"), (0, [(4, 4)], b"0 <= from < to"), (0, [(-1, 4)], b"0 <= from < to"),
                                (2, [(0, 1)], b"no such event bank source"), (-2, [], b"no such event bank source"), (-1, [(0, 1)], b"only clears")]:
        with pytest.raises(host.HipError):
            bank.set_daylight(source, spans)
        assert text in lib.bnhip_last_error(), (source, spans, lib.bnhip_last_error())
    assert lib.bnhip_event_bank_set_daylight(bank._h, 0, None, 1) == host.E_INVALID
    with pytest.raises(host.HipError, match="dog_remember_windows"):
        bank.set_guards(host.EventGuards(None, 0.5, None, -1, None))
    with pytest.raises(host.HipError, match="n_classes"):
        bank.set_guards(host.EventGuards(np.zeros(n - 1, np.uint8)))
    assert np.array_equal(bank.pending(), before)
    assert bank.flush()["first_window"].size == 0                        # the settings stood: both events began in daylight
    bank.close()


# ------------------------------------------------------------------------------------------ through the model
def test_fused_tick_guarded(gpu, tiny_cfg, tiny_blob):
    """bnhip_windows_predict_events with guards set on its bank: the tick's events are those of a second bank under the same guards
    fed the tick's own out_conf / out_idx through process."""
    from birdnet_go_amd import stream as S
    clf = host.HipClassifier(tiny_blob, device=0, max_batch=8)
    nc, k, hold, n_ticks, n_src = clf.num_species(), 5, 2, 5, 3
    clip_bytes = tiny_cfg.n_samples * 2
    overlap, read = clip_bytes // 2, clip_bytes - clip_bytes // 2
    w = S.NativeWindows(overlap, read, max_batch=256)
    rng = np.random.default_rng(11)
    pcm = (rng.normal(0, 0.2, (n_src, n_ticks * read // 2)).clip(-1, 1) * 32767).astype("<i2")
    for s in range(n_src):
        assert w.add_source(f"mic{s}", 2 * n_ticks * clip_bytes) == s
        w.write(s, pcm[s])
    kk = min(k, nc)
    flt = host.EventTables(np.full(nc, -1.0, np.float32), None, 0.0, hold, 1, host.EVENTS_KEEP_DROPPED)
    # every class the model ranks is a dog hit; the even classes are dropped by it, the odd ones in source 1's daylight
    g = host.EventGuards(np.ones(nc, np.uint8), -1.0, (np.arange(nc) % 2 == 0).astype(np.uint8), 2, (np.arange(nc) % 2 == 1).astype(np.uint8))
    fused, fed = host.EventBank(nc, kk, flt, 8, guards=g), host.EventBank(nc, kk, flt, 8, guards=g)
    for b in (fused, fed):
        b.set_daylight(1, [(0, 2), (3, 4)])
    saw = set()
    for _ in range(n_ticks):
        idxs, rows, conf, idx, events = clf.predict_windows_events(w, fused, 16, k, 0, 1.0)
        assert idxs == list(range(n_src))
        assert np.array_equal(events, fed.process(idxs, conf, idx))
        saw |= set(events["status"].tolist())
    assert np.array_equal(fused.pending(), fed.pending()) and np.array_equal(fused.flush(), fed.flush())
    assert saw == {KEPT, DOG, DAYLIGHT}                                  # (an even class always has its bark; an odd one of source 1 its daylight)
    for b in (fused, fed):
        b.close()
    w.close()
    clf.close()


def test_fused_channels_guarded(gpu):
    """Two short recordings through bnhip_analyze_channels_pcm_events_guarded: the guarded tail over the rows of the _pcm entry; and
    bnhip_analyze_channels_pcm_clips_guarded: a clip for each status-0 event and for no other."""
    clf = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False)
    xs = _recordings([14 * CLIP + 3, 9 * CLIP], seed=47)
    raw = b"".join(_bytes(x, 16) for x in xs)
    recs = host.channel_recordings([x.size for x in xs], 48000, 16, 1, 0)
    rows, _, chosen = clf.analyze_channels_pcm(raw, recs, 48000, HOP, MIN_TAIL, k=K, threshold=0.0)
    nc = clf.num_species()
    seen = np.unique(rows["class_index"])
    assert seen.size >= 3
    dog = np.zeros(nc, np.uint8)
    dog[seen[0]] = 1
    filtered, day = np.zeros(nc, np.uint8), np.zeros(nc, np.uint8)
    filtered[seen[1::2]], day[seen[2::2]] = 1, 1
    g = host.EventGuards(dog, float(np.median(rows["confidence"][rows["class_index"] == seen[0]])), filtered, 2, day,
                         np.array([(0, 2, 6), (0, 9, 11), (1, 0, 3)], np.int32))
    ext = host.EventExtend(None, **dict(SMALL, max_windows=9))
    for x in (None, ext):
        f = host.EventTables(np.full(nc, -1.0, np.float32), None, 0.0, 2, 1, host.EVENTS_KEEP_DROPPED)
        want = guardref.events(rows, f, x, g)
        assert {KEPT, DOG, DAYLIGHT} <= set(want["status"].tolist())
        got, chosen_ev = clf.analyze_channels_pcm_events(raw, recs, 48000, HOP, f, MIN_TAIL, k=K, extend=x, guards=g)
        assert np.array_equal(got, want) and chosen_ev.tolist() == chosen.tolist()
        assert np.array_equal(host.detection_events(rows, nc, f, extend=x, guards=g), want)
        f0 = host.EventTables(f.class_threshold, None, 0.0, 2, 1, 0)
        kept = want[want["status"] == KEPT]
        settings = host.ClipSettings(5000, 15001, 40 * CLIP, x is not None, False, lpc_order=8)
        clips = clf.analyze_channels_pcm_clips(raw, recs, 48000, HOP, f0, settings, MIN_TAIL, k=K, extend=x, guards=g)
        assert np.array_equal(clips.events, kept) and clips.n_clips == kept.size == len(clips.flac)
        assert np.array_equal(clips.spans, host.event_clip_spans(kept, [x_.size for x_ in xs], HOP, settings))
        unguarded = clf.analyze_channels_pcm_clips(raw, recs, 48000, HOP, f0, settings, MIN_TAIL, k=K, extend=x)
        assert unguarded.n_clips == want.size > kept.size
    with pytest.raises(host.HipError, match="recording outside the call"):
        clf.analyze_channels_pcm_events(raw, recs, 48000, HOP, f, MIN_TAIL, k=K,
                                        guards=host.EventGuards(None, 0.0, None, 0, day, np.array([(2, 0, 3)], np.int32)))
    clf.close()


@pytest.mark.parametrize("which", ["dog", "daylight"])
def test_dynamic_bank_does_not_learn_from_a_dropped_event(gpu, which):
    """One source, one event of class 1 at 0.9 above the trigger 0.7: approved, it takes class 1 to level 1; dropped by either guard it
    is not approved - no change record, level 0."""
    n, k, hold = 8, 2, 2
    thr = np.full(n, 0.5, np.float32)
    thr[6] = np.inf                                                      # the dog class forms no event of its own here
    flt = host.EventTables(thr, None, 0.0, hold, 1, host.EVENTS_KEEP_DROPPED)
    t = lambda cs: np.isin(np.arange(n), cs).astype(np.uint8)
    g = host.EventGuards(t([6]), 0.6, t([1]), 5, None) if which == "dog" else host.EventGuards(None, 0.0, None, 0, t([1]))
    conf = np.array([[0.9, 0.7], [0.0, 0.0]], np.float32)
    idx = np.array([[1, 6], [-1, -1]], np.int32)
    for guards, status, level in [(None, KEPT, 1), (g, DOG if which == "dog" else DAYLIGHT, 0)]:
        bank = host.EventBank(n, k, flt, 1, dynamic=host.EventDynamic(None, 0.7, 0.1, 100, 0), guards=guards)
        bank.set_daylight(0, [(0, 1)])
        bank.set_now(10)
        ev = bank.process([0, 0], conf, idx)
        assert ev["status"].tolist() == [status] and ev["class_index"].tolist() == [1]
        changes = bank.threshold_changes()
        assert bank.thresholds()[0][1] == level and changes.size == level
        assert not level or (changes[0]["class_index"], changes[0]["reason"]) == (1, host.THRESHOLD_HIGH_CONFIDENCE)
        bank.close()


def test_analyze_files_guards(gpu, tmp_path):
    """wav.analyze_files(events=, guards=) takes the channels route and answers the tuples of the restatement's events: the dog class
    found among the labels, species by label and by index, minutes and seconds in windows."""
    from birdnet_go_amd import wav
    from test_analyze import _write_wav16
    clf = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False)
    (x,) = _recordings([14 * CLIP + 3], seed=53)
    path = str(tmp_path / "r.wav")
    _write_wav16(path, x)
    rate, nc = 48000, clf.num_species()
    clip_seconds, overlap = CLIP / rate, (CLIP - HOP) / rate
    recs = host.channel_recordings([x.size], rate, 16, 1, 0)
    clip_len, hop, min_tail = wav._framing(rate, clip_seconds, overlap, 1.0)
    assert (clip_len, hop) == (CLIP, HOP)
    rows, _, _ = clf.analyze_channels_pcm(_bytes(x, 16), recs, rate, HOP, min_tail, k=K, threshold=0.0)
    seen = np.unique(rows["class_index"])
    labels = [f"sp{i}_Bird {i}" for i in range(nc)]
    labels[seen[0]] = "Dog_Hund"
    flt = wav.EventFilter(default_threshold=-1.0, hold_seconds=2 * HOP / rate, keep_dropped=True)
    g = wav.EventGuards(float(np.median(rows["confidence"][rows["class_index"] == seen[0]])), species=[labels[c] for c in seen[1::2]],
                        remember_minutes=1.9 * HOP / rate / 60, daylight_species=[int(c) for c in seen[2::2]],
                        daylight={path: [(1.5 * HOP / rate, 5.5 * HOP / rate), (8.5 * HOP / rate, 10.5 * HOP / rate)]})
    tables, gt = flt.tables(nc, rate, HOP, overlap), g.tables(nc, rate, HOP, labels, [path])
    assert gt.class_dog.nonzero()[0].tolist() == [seen[0]] and gt.dog_remember_windows == 2 and gt.daylight_spans.tolist() == [[0, 2, 6], [0, 9, 11]]
    ev = guardref.events(rows, tables, None, gt)
    assert {KEPT, DOG, DAYLIGHT} <= set(ev["status"].tolist())
    want = [(float(np.float64(int(e["first_window"]) * HOP) / rate), float(np.float64(int(e["last_window"]) * HOP) / rate + clip_seconds),
             labels[int(e["class_index"])], float(e["confidence"]), int(e["count"]), int(e["status"])) for e in ev]
    kw = dict(labels=labels, overlap_seconds=overlap, top_k=K, model_rate=rate, events=flt)
    assert wav.analyze_files([path], clf, guards=g, **kw) == [want]
    assert wav.analyze_files([path], clf, **kw) != [want]
    clf.close()


def test_window_batcher_guards(gpu, tiny_cfg, tiny_blob):
    """WindowBatcher(events=, guards=) sets the guards on the model's bank when it creates it, with the daylight that was set
    before; the ticks' events are the restatement's fed the Results' own rows."""
    from birdnet_go_amd import results as R, stream as S
    clf = host.HipClassifier(tiny_blob, device=0, max_batch=8)
    nc = clf.num_species()
    labels = [f"sp{i}" for i in range(nc)]
    bn = host.BirdNET(clf, labels, sensitivity=1.0)
    n, rate = tiny_cfg.n_samples, tiny_cfg.sample_rate
    spec = S.ModelSpec(rate, 3.0, clip_bytes=n * 2)
    hop = n - n // 2
    flt = host.EventTables(np.full(nc, -1.0, np.float32), None, 0.0, 2, 1, evref.KEEP_DROPPED)
    g = host.EventGuards(np.ones(nc, np.uint8), -1.0, (np.arange(nc) % 2 == 0).astype(np.uint8), 2, (np.arange(nc) % 2 == 1).astype(np.uint8))
    rng = np.random.default_rng(29)
    n_src, n_win = 2, 8
    t = np.arange(hop * (n_win + 1)) / rate
    streams = {f"src{i}": (np.clip(0.4 * np.sin(2 * np.pi * (600 + 400 * i) * t) + rng.normal(0, 0.05, t.size), -1, 1) * 32767).astype("<i2").tobytes()
               for i in range(n_src)}
    o = S.Orchestrator()
    o.register("tiny", bn, spec)
    wb = S.WindowBatcher(o, R.ResultsQueue(size=1000), max_batch=8, events=flt, guards=g)
    for s in streams:
        wb.allocate(s, "tiny")
    # windows 2, 3 and 5 of src1 begin in [1.5 hop, 3.2 hop) or [4.1 hop, 5.5 hop): both edges up to the next window start
    wb.set_daylight("src1", [(1.5 * hop / rate, 3.2 * hop / rate), (4.1 * hop / rate, 5.5 * hop / rate)])
    assert wb.daylight[("tiny", wb.buffers[("src1", "tiny")].index)] == [(2, 4), (5, 6)]
    for lo in range(0, len(t) * 2, 5000):
        for s, b in streams.items():
            wb.write(s, b[lo:lo + 5000])
        wb.tick()
    while wb.tick():
        pass
    taken = wb.take_events()
    msgs = []
    while wb.queue.qsize():
        msgs.append(wb.queue.get())
    ref = guardref.EventBank(n_src, nc, min(10, nc), flt, None, g)
    ref.set_daylight(1, [(2, 4), (5, 6)])
    want = []
    for m in msgs:
        conf, idx = np.full((1, ref.k), np.nan, np.float32), np.full((1, ref.k), -1, np.int32)
        for j, d in enumerate(m.results):
            conf[0, j], idx[0, j] = d.confidence, labels.index(d.species)
        want += [(f"src{e['recording']}", int(e["class_index"]), int(e["first_window"]), int(e["status"])) for e in ref.process([int(m.source[3:])], conf, idx)]
    got = [(e["source"], e["class_index"], e["first_window"], e["status"]) for e in taken]
    assert sorted(got) == sorted(want) and {e["status"] for e in taken} == {KEPT, DOG, DAYLIGHT}
    assert {e["first_window"] for e in taken if e["status"] == DAYLIGHT} <= {2, 3, 5}
    wb.set_guards(None)
    wb.close()
    clf.close()
