"""Extended capture on the device: an extended event bank and the extended file tail over crafted rows, every answer np.array_equal
to the restatement (tests/evxref.py) - the rule is compares and integer arithmetic, so there is no tolerance to choose - and then
through the tiny models: the fused analysis entry and WindowBatcher(events=, extend=, capture=)."""
import ctypes as C

import numpy as np
import pytest

from birdnet_go_amd import flac, host, wav

import capref
import evref
import evxref
from test_analyze import CLIP, HOP, K, MIN_TAIL, _bytes, _fft_tiny_blob, _recordings, _write_wav16
from test_event_bank import Pair
from test_event_bank_ref import by_key, detection_rows, feed, filters, topk_rows

pytestmark = pytest.mark.gpu

# every stage inside 14 windows; with hold 3 the short stage waits 3
SMALL = dict(max_windows=14, short_wait=2, medium_from=5, medium_wait=4, long_from=9, long_wait=6)


def extend(table=None, **kw):
    return host.EventExtend(table, **dict(SMALL, **kw))


class XPair(Pair):
    """An extended device bank and the streaming restatement side by side (test_event_bank.Pair with the extend)."""

    def __init__(self, max_sources, n_classes, k, flt, ext):
        self.dev = host.EventBank(n_classes, k, flt, max_sources, extend=ext)
        self.ref = evxref.EventBank(max_sources, n_classes, k, flt, ext)
        self.n_classes, self.flt, self.ext = n_classes, flt, ext
        assert self.dev.extended and self.dev.slots_per_source == self.ref.slots_per_source and self.dev.hold_windows == flt.hold_windows
        self.answers = []

    def set_extend(self, ext):
        self.dev.set_extend(ext)
        self.ref.set_extend(ext)
        self.ext = ext

    def flushed_is_one_shot(self, conf, idx):
        """Flushes; everything answered so far is then what the extended tail finds in the joined rows, which is the restatement's."""
        self.flush()
        assert self.pending().size == 0
        rows = detection_rows(conf, idx)
        want = host.detection_events(rows, self.n_classes, self.flt, extend=self.ext)
        assert np.array_equal(want, evxref.events(rows, self.flt, self.ext))
        assert np.array_equal(by_key(self.answers), want)
        return want


def plain_filter(n_classes, hold, min_count=1, flags=0, veto=None):
    return host.EventTables(np.full(n_classes, 0.5, np.float32), veto, 0.5, hold, min_count, flags)


def spans(ev, cls=None):
    return [(int(e["first_window"]), int(e["last_window"]), int(e["count"])) for e in ev if cls is None or e["class_index"] == cls]


# ------------------------------------------------------------------------------------------ the bank, small
def test_bank_small(gpu):
    """n_classes 6, k 2, hold 3: class 3 slides, class 4 does not.  Source 0: a hit at d - 1 joins and the hit at the new d opens the
    next event.  Source 1: the same across medium_from and long_from and up to the cap.  Source 2: class 3 in every window ends at
    b + max_windows - 1 and reopens at b + max_windows.  Source 3: a sliding and a fixed class side by side.  One call, one window per
    call, and two calls split at every boundary."""
    n_classes, k, hold, n_win = 6, 2, 3, 32
    table = np.array([1, 1, 1, 1, 0, 1], np.uint8)
    idx = np.full((4, n_win, k), -1, np.int32)
    conf = np.full(idx.shape, 0.75, np.float32)
    for w in (1, 3, 6):                              # b = 1: d = 4; the hit at 3 = d - 1 joins, d = 6; the hit at 6 opens the next
        idx[0, w, 0] = 3
    # b = 0: d = 3; 2 joins, d = 5; 4 joins, d = 7; 6 (t >= 5: medium) joins, d = 10; 9 = d - 1 (t >= 9: long) joins, d = min(15, 14);
    # 13 = d - 1 joins, d stays 14; 14 opens the next
    for w in (0, 2, 4, 6, 9, 13, 14):
        idx[1, w, 1] = 3
    idx[2, :, 0] = 3
    idx[3, :, 0], idx[3, :, 1] = 4, 3
    idx[3, 20:22] = -1                               # a gap: class 3's deadline (19 + 4 = 23: the medium stage of b = 14) bridges it
    conf[3, 5], conf[3, 17] = 0.875, 0.9375
    want = None
    for plan in ["all", "window"] + list(range(1, n_win)):               # a number: two calls, split in front of that window
        p = XPair(4, n_classes, k, plain_filter(n_classes, hold), extend(table))
        if plan == "all":
            calls = feed(p, conf, idx, "all", np.random.default_rng(0))
            assert len(calls) == 1
        elif plan == "window":
            calls = feed(p, conf, idx, "window")
            assert len(calls) == n_win and all(lo == hi for _, span in calls for lo, hi in span.values())
        else:
            for lo, hi in ((0, plan), (plan, n_win)):
                src = [s for w in range(lo, hi) for s in range(4)]
                p.process(src, conf[:, lo:hi].transpose(1, 0, 2).reshape(-1, k), idx[:, lo:hi].transpose(1, 0, 2).reshape(-1, k))
        got = p.flushed_is_one_shot(conf, idx)
        assert want is None or np.array_equal(got, want)
        want = got if want is None else want
        p.close()
    by = lambda s, c: spans(want[want["recording"] == s], c)
    assert by(0, 3) == [(1, 3, 2), (6, 6, 1)]
    assert by(1, 3) == [(0, 13, 6), (14, 14, 1)]
    assert by(2, 3) == [(0, 13, 14), (14, 27, 14), (28, 31, 4)]
    assert by(3, 3) == [(0, 13, 14), (14, 27, 12), (28, 31, 4)]
    assert by(3, 4)[:3] == [(0, 2, 3), (3, 5, 3), (6, 8, 3)] and all(b - a < hold for a, b, _ in by(3, 4))


# ------------------------------------------------------------------------------------------ slots
@pytest.mark.parametrize("k,W,hold", [(10, 7, 4), (64, 64, 33)])
def test_every_slot_live_at_once(gpu, k, W, hold):
    """slots_per_source = k * W with W = long_wait, beyond k * hold: 70 (several lane steps) and 4096 (112 KiB of LDS).  With
    medium_from = long_from = 1 a second hit gives an event long_wait.  Windows 0 .. W - hold - 1 open k classes each; the next
    W - hold windows hit them again, in the same order, hold - 1 windows before they would run out, and live on W windows from there; the
    last hold windows open k new classes each.  While window w* = 2 W - hold - 1 is applied every one of the k * W slots is live, and
    it frees the first group of either kind; the classes freed then come round again.  Source 1 numbers its classes from the top."""
    S, n_classes = hold, k * W
    assert W <= 2 * S - 1 and k * S < k * W
    last = 2 * W - S - 1
    n_win = last + 3
    group = [g for g in range(W - S)] * 2 + [W - S + j for j in range(S)]        # window -> the group it brings
    group += [0, W - S, 1]                                                       # freed after w*, w*, w* + 1
    idx = np.full((2, n_win, k), -1, np.int32)
    for w in range(n_win):
        idx[0, w] = group[w] * k + np.arange(k)
        idx[1, w] = n_classes - 1 - (group[w] * k + np.arange(k))
    conf = np.full(idx.shape, 0.75, np.float32)
    conf[:, 1::2] = 0.875
    ext = host.EventExtend(None, max_windows=4 * W, short_wait=1, medium_from=1, medium_wait=W, long_from=1, long_wait=W)
    p = XPair(2, n_classes, k, plain_filter(n_classes, hold), ext)
    assert p.dev.slots_per_source == k * W
    feed(p, conf[:, :last], idx[:, :last], "all")
    assert p.pending().size == 2 * k * (W - 1)
    got = p.process([1, 0], conf[::-1, last], idx[::-1, last])                   # every slot live, then two groups freed
    assert got.size == 2 * 2 * k and set(got["first_window"]) == {0, 2 * (W - S)}
    for w in range(last + 1, n_win):
        p.process([0, 1], conf[:, w], idx[:, w])
    p.flushed_is_one_shot(conf, idx)
    p.close()


# ------------------------------------------------------------------------------------------ veto
def test_veto_against_the_final_deadline(gpu):
    """Class 2 hits at 3, 5 and 7 with hold 3: it slid twice, d = 6, 8, 10, and its three hits reach min_count 3, which no fixed hold
    would give.  The source's veto hit lies at b - 1, b, d - 1 or d: vetoed for the two inside.  Class 3 hits once: status 1."""
    n_classes, k, hold, b, d = 5, 2, 3, 3, 10
    veto = np.array([1, 0, 0, 0, 0], np.uint8)
    idx = np.full((4, d + 3, k), -1, np.int32)
    conf = np.full(idx.shape, 0.75, np.float32)
    for s, v in enumerate([b - 1, b, d - 1, d]):
        idx[s, [3, 5, 7], 0] = 2
        idx[s, 4, 1] = 3
        idx[s, v, 1] = 0
    for plan in ("window", "all"):
        p = XPair(4, n_classes, k, plain_filter(n_classes, hold, min_count=3, flags=evref.KEEP_DROPPED, veto=veto), extend())
        feed(p, conf, idx, plan, np.random.default_rng(0))
        want = p.flushed_is_one_shot(conf, idx)
        assert spans(want, 2) == [(3, 7, 3)] * 4
        assert want[want["class_index"] == 2]["status"].tolist() == [0, 2, 2, 0]
        assert want[want["class_index"] == 3]["status"].tolist() == [1, 1, 1, 1]
        p.close()


# ------------------------------------------------------------------------------------------ set_extend
def test_set_extend_mid_stream(gpu):
    n_classes, k, hold = 6, 2, 3
    flt = plain_filter(n_classes, hold)
    p = XPair(1, n_classes, k, flt, extend())
    hit = lambda *cls: (np.full((1, k), 0.75, np.float32), np.array([list(cls) + [-1] * (k - len(cls))], np.int32))
    p.process([0], *hit(1, 2))                                           # window 0: both due at 3
    p.set_extend(None)                                                   # sliding off from the next call
    p.process([0], *hit(1))                                              # window 1: class 1 joins and keeps its deadline
    assert spans(p.process([0], *hit())) == [(0, 1, 2), (0, 0, 1)]       # window 2: both answered
    only2 = np.array([0, 0, 1, 0, 0, 0], np.uint8)
    p.set_extend(extend(only2))                                          # a new table: class 2 slides, class 1 does not
    p.process([0], *hit(1, 2))                                           # window 3: both due at 6
    p.process([0], *hit(1, 2))                                           # window 4: class 2 slides to 7
    assert p.process([0], *hit())["class_index"].tolist() == [1]         # window 5: class 1 answered, class 2 not
    assert spans(p.pending()) == [(3, 4, 2)]
    p.set_extend(extend(None, short_wait=6))                             # every class, and the short stage waits 6 - from the next hit on
    assert spans(p.process([0], *hit())) == [(3, 4, 2)]                  # window 6: class 2 kept the deadline 7 its last hit gave it
    p.process([0], *hit(2))                                              # window 7: opens, due at 13
    for _ in range(4):
        assert p.process([0], *hit()).size == 0                          # windows 8 .. 11
    before = p.pending()
    assert spans(before) == [(7, 7, 1)]
    for bad in (extend(None, long_wait=7), extend(None, short_wait=7), extend(None, max_windows=2), extend(np.zeros(5, np.uint8))):
        with pytest.raises(host.HipError):
            p.dev.set_extend(bad)
        assert np.array_equal(p.dev.pending(), before)
    lib = host._event_bank_protos(host.load_library())
    xs = extend(None, medium_wait=9)._struct(n_classes)
    assert lib.bnhip_event_bank_set_extend(p.dev._h, C.addressof(xs)) == host.E_INVALID and b"longest wait" in lib.bnhip_last_error()
    assert spans(p.process([0], *hit())) == [(7, 7, 1)]                  # window 12: 13 <= 12 + 1
    p.close()
    plain = host.EventBank(n_classes, k, flt, 1)
    assert not plain.extended
    with pytest.raises(host.HipError, match="without an extend"):
        plain.set_extend(extend())
    with pytest.raises(host.HipError, match="without an extend"):
        plain.set_extend(None)
    plain.close()


# ------------------------------------------------------------------------------------------ transactions
def test_failed_call_changes_nothing(gpu):
    """A call that slides one deadline, opens and answers events, with cap one below the need: BNHIP_E_INVALID, the need in
    .needed, pending and the clock as before; the same call with room then answers the restatement's bytes, and so does the rest of
    the stream - the deadlines were where they had been."""
    n_classes, k, hold, n_win = 8, 4, 2, 9
    idx = np.full((1, n_win, k), -1, np.int32)
    conf = np.full(idx.shape, 0.75, np.float32)
    idx[0, 0] = [0, 1, 2, 3]                          # due at 2
    idx[0, 1] = [0, 4, 5, -1]                         # class 0 slides to 3; 4 and 5 due at 3
    idx[0, 2] = [0, 6, -1, -1]                        # class 0 slides to 4
    idx[0, 5] = [0, 1, -1, -1]
    p = XPair(1, n_classes, k, plain_filter(n_classes, hold), extend())
    p.process([0], conf[0, 0], idx[0, 0])
    before = p.pending()
    assert before.size == 4
    want = p.ref.process([0, 0, 0], conf[0, 1:4], idx[0, 1:4])
    assert want.size == 7                             # 1, 2, 3 after window 1; 4, 5 after window 2; 0 and 6 after window 3
    with pytest.raises(host.HipError) as ei:
        p.dev.process([0, 0, 0], conf[0, 1:4], idx[0, 1:4], cap=want.size - 1)
    assert ei.value.needed == want.size and np.array_equal(p.dev.pending(), before) and p.dev.clock(0) == 1
    got = p.dev.process([0, 0, 0], conf[0, 1:4], idx[0, 1:4], cap=want.size)
    assert np.array_equal(got, want) and p.dev.clock(0) == 4
    p.answers.append(got)
    feed_from = 4
    for w in range(feed_from, n_win):
        p.process([0], conf[0, w], idx[0, w])
    p.flushed_is_one_shot(conf, idx)
    p.close()


# ------------------------------------------------------------------------------------------ the rule on random rows
@pytest.mark.parametrize("hold", [1, 3, 8])
@pytest.mark.parametrize("plan", ["window", "all", "groups"])
def test_random_rows(gpu, hold, plan):
    """The inputs of test_event_bank.test_random_rows - ties, == threshold, NaN confidences, +inf and NaN thresholds, veto classes,
    empty windows, sources absent from a call - with half the classes sliding."""
    longest = 0
    for min_count, flags in [(1, 0), (3, evref.KEEP_DROPPED), (3, 0)]:
        rng = np.random.default_rng(100 * hold + min_count + flags)
        n_src, n_win, n_classes, k = 4, 24, 14, 4
        conf, idx = topk_rows(rng, n_src, n_win, n_classes, k)
        table = (rng.random(n_classes) < 0.5).astype(np.uint8)
        table[3], table[4] = 1, 0
        p = XPair(n_src + 1, n_classes, k, filters(rng, n_classes, hold, min_count, True, flags), extend(table))
        feed(p, conf, idx, plan, np.random.default_rng(hold))
        p.pending()
        assert p.clocks(range(n_src + 1)) == [n_win] * n_src + [0]
        want = p.flushed_is_one_shot(conf, idx)
        assert want.size or (min_count > 1 and not flags)
        longest = max([longest] + (want["last_window"] - want["first_window"]).tolist())
        p.close()
    assert longest >= hold                                               # (of the input: an event no fixed hold could give)


# ------------------------------------------------------------------------------------------ the file tail
def _rows(items):
    rows = np.zeros(len(items), host.DETECTION)
    for i, q in enumerate(items):
        rows[i] = q
    return rows[np.lexsort((rows["window"], rows["recording"]))]


def _tail(rows, n_classes, ext, hold=3, **kw):
    """The extended device tail against the restatement, dropped events left out and kept; -> the events with their statuses."""
    for flags in (0, host.EVENTS_KEEP_DROPPED):
        f = host.EventTables(np.full(n_classes, 0.5, np.float32), kw.get("veto"), 0.5, hold, kw.get("min_count", 1), flags)
        got, want = host.detection_events(rows, n_classes, f, extend=ext), evxref.events(rows, f, ext)
        assert got.dtype == evref.EVENT and np.array_equal(got, want), (flags, got, want)
    return got


def test_tail_cap_across_steps(gpu):
    """One class in 130 consecutive windows, max_windows 50: events at 0, 50 and 100 - the walk crosses the 64-hit step with the
    predecessor carried, and the second event begins before the step boundary and ends behind it."""
    ev = _tail(_rows([(0, w, 0, 0.75) for w in range(130)]), 1, extend(max_windows=50))
    assert spans(ev) == [(0, 49, 50), (50, 99, 50), (100, 129, 30)]


@pytest.mark.parametrize("at", [63, 64, 65])
@pytest.mark.parametrize("joins", [False, True])
def test_tail_boundary_at_a_step_edge(gpu, at, joins):
    """Hits 0 .. at - 1 in consecutive windows; hit `at` lies at the deadline the hit before it gave (it opens the next event) or
    one window earlier (it joins): on the last lane of a step, on lane 0 of the next - judged against the carried predecessor - and
    on lane 1."""
    ext = extend(max_windows=400)
    d = evxref.deadline(0, at - 1, 3, ext)
    assert d == at - 1 + 6
    nxt = d - 1 if joins else d
    ev = _tail(_rows([(0, w, 0, 0.75) for w in range(at)] + [(0, nxt + j, 0, 0.75) for j in range(70)]), 1, ext)
    assert spans(ev) == ([(0, nxt + 69, at + 70)] if joins else [(0, at - 1, at), (nxt, nxt + 69, 70)])


def test_tail_group_across_a_block(gpu):
    """Two recordings' groups of 200 hits with gaps: sorted, the second group runs from hit 200 to hit 399, across row 256 - the
    wave that owns its head walks into the next block's hits."""
    items = []
    for r in range(2):
        w = 0
        for j in range(200):
            items.append((r, w, 2, 0.75))
            w += 1 + (j % 9 == r) * 7                # now and then a gap beyond every wait
    ev = _tail(_rows(items), 3, extend(max_windows=60))
    assert (ev["recording"] == 1).sum() > 3 and int(ev[ev["recording"] == 1]["count"].sum()) == 200


def test_tail_64_groups_in_one_wave(gpu):
    """64 classes hit once each in window 0 and a 65th in 100 windows: sorted, the first wave holds 64 group heads."""
    items = [(0, 0, c, 0.75) for c in range(64)] + [(0, w, 64, 0.75) for w in range(100)]
    ev = _tail(_rows(items), 65, extend(max_windows=30))
    assert ev.size == 64 + 4 and spans(ev, 64) == [(0, 29, 30), (30, 59, 30), (60, 89, 30), (90, 99, 10)]


def test_tail_mixed_classes_and_veto(gpu):
    rng = np.random.default_rng(8)
    n_classes = 10
    table = np.array([0, 1] * 5, np.uint8)
    veto = np.zeros(n_classes, np.uint8)
    veto[9] = 1
    items = [(r, w, int(c), float(rng.integers(20, 64)) / 64.0) for r in range(3) for w in range(300) for c in rng.permutation(n_classes)[:3]]
    ev = _tail(_rows(items), n_classes, extend(table), hold=2, veto=veto, min_count=2)
    assert set(ev["status"]) == {0, 1, 2}


def test_tail_no_sliding_class_is_the_plain_entry(gpu):
    rng = np.random.default_rng(3)
    n_src, n_win, n_classes, k = 3, 80, 12, 4
    conf, idx = topk_rows(rng, n_src, n_win, n_classes, k)
    rows = detection_rows(conf, idx)
    for hold in (1, 3, 8):
        f = filters(rng, n_classes, hold, 2, True, evref.KEEP_DROPPED)
        plain = host.detection_events(rows, n_classes, f)
        zero = host.detection_events(rows, n_classes, f, extend=extend(np.zeros(n_classes, np.uint8)))
        assert plain.size and zero.tobytes() == plain.tobytes()
        assert host.detection_events(rows, n_classes, f, extend=extend()).tobytes() != plain.tobytes()
        # ... and a bank created extended with such a table answers the bytes of one created without
        banks = [host.EventBank(n_classes, k, f, n_src), host.EventBank(n_classes, k, f, n_src, extend=extend(np.zeros(n_classes, np.uint8)))]
        answers = [b"".join(c[0].tobytes() for c in feed(b, conf, idx, "groups", np.random.default_rng(5))) + b.flush().tobytes() for b in banks]
        assert answers[0] == answers[1]
        for b in banks:
            b.close()


# ------------------------------------------------------------------------------------------ through the model
def test_fused_channels_extended(gpu):
    """One short recording through bnhip_analyze_channels_pcm_events_extended: the extended tail over the rows of the _pcm entry."""
    clf = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False)
    (x,) = _recordings([14 * CLIP + 3], seed=41)
    raw = _bytes(x, 16)
    recs = host.channel_recordings([x.size], 48000, 16, 1, 0)
    rows, _, chosen = clf.analyze_channels_pcm(raw, recs, 48000, HOP, MIN_TAIL, k=K, threshold=0.0)
    nc = clf.num_species()
    thr = np.full(nc, np.inf, np.float32)
    for c in np.unique(rows["class_index"]):
        v = np.unique(rows["confidence"][rows["class_index"] == c])
        thr[c] = np.float32(-1.0) if v.size < 2 else np.float32((float(v[0]) + float(v[1])) / 2)      # all but a class's weakest hit
    f = host.EventTables(thr, None, 0.0, 2, 1, host.EVENTS_KEEP_DROPPED)
    table = np.zeros(nc, np.uint8)
    table[::2] = 1
    ext = extend(table, max_windows=9)
    want = evxref.events(rows, f, ext)
    assert want.size and (want["last_window"] - want["first_window"]).max() >= 2
    got, chosen_ev = clf.analyze_channels_pcm_events(raw, recs, 48000, HOP, f, MIN_TAIL, k=K, extend=ext)
    assert np.array_equal(got, want) and chosen_ev.tolist() == chosen.tolist()
    assert np.array_equal(host.detection_events(rows, nc, f, extend=ext), want)
    assert not np.array_equal(clf.analyze_channels_pcm_events(raw, recs, 48000, HOP, f, MIN_TAIL, k=K)[0], want)
    # ... and bnhip_analyze_channels_pcm_clips_extended: the same events (kept ones only), each clip cut to its event's last hit
    f0 = host.EventTables(thr, None, 0.0, 2, 1, 0)
    kept = evxref.events(rows, f0, ext)
    xs = host.ClipSettings(5000, 15001, 40 * CLIP, True, False, lpc_order=8)
    clips = clf.analyze_channels_pcm_clips(raw, recs, 48000, HOP, f0, xs, MIN_TAIL, k=K, extend=ext)
    cut = host.event_clip_spans(kept, [x.size], HOP, xs)
    assert np.array_equal(clips.events, kept) and np.array_equal(clips.spans, cut) and clips.n_clips == kept.size
    pcm = np.frombuffer(raw, "<i2")
    longest = int(np.argmax(kept["last_window"] - kept["first_window"]))
    assert cut[longest]["length"] == min(x.size, int(kept[longest]["last_window"]) * HOP + 15001) - max(0, int(kept[longest]["first_window"]) * HOP - 5000)
    for dec, sp in zip(flac.decode_clips(clips.flac)[0], cut):
        assert np.array_equal(dec, pcm[int(sp["start"]):int(sp["start"]) + int(sp["length"])])
    clf.close()


def test_analyze_files_extend(gpu, tmp_path):
    """wav.analyze_files(events=, extend=) takes the channels route and answers the tuples of the restatement's events; with an
    extended export every tuple carries the span bnhip_event_clip_spans gives its event."""
    clf = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False)
    (x,) = _recordings([14 * CLIP + 3], seed=43)
    path = str(tmp_path / "r.wav")
    _write_wav16(path, x)
    rate, nc = 48000, clf.num_species()
    clip_seconds, overlap = CLIP / rate, (CLIP - HOP) / rate
    recs = host.channel_recordings([x.size], rate, 16, 1, 0)
    clip_len, hop, min_tail = wav._framing(rate, clip_seconds, overlap, 1.0)
    assert (clip_len, hop) == (CLIP, HOP)
    rows, _, _ = clf.analyze_channels_pcm(_bytes(x, 16), recs, rate, HOP, min_tail, k=K, threshold=0.0)
    flt = wav.EventFilter(default_threshold=-1.0, hold_seconds=2 * HOP / rate)
    cap = wav.ExtendedCapture(species=list(range(0, nc, 2)), max_seconds=9 * HOP / rate, short_wait_seconds=2 * HOP / rate,
                              medium_after_seconds=5 * HOP / rate, medium_wait_seconds=4 * HOP / rate, long_after_seconds=8 * HOP / rate,
                              long_wait_seconds=6 * HOP / rate)
    tables, ext = flt.tables(nc, rate, HOP, overlap), cap.tables(nc, rate, HOP)
    assert (tables.hold_windows, ext.max_windows, ext.short_wait, ext.medium_from, ext.medium_wait, ext.long_from, ext.long_wait) == (2, 9, 2, 5, 4, 8, 6)
    ev = evxref.events(rows, tables, ext)
    assert ev.size and (ev["last_window"] - ev["first_window"]).max() >= 2
    want = [(float(np.float64(int(e["first_window"]) * HOP) / rate), float(np.float64(int(e["last_window"]) * HOP) / rate + clip_seconds),
             int(e["class_index"]), float(e["confidence"]), int(e["count"])) for e in ev]
    kw = dict(overlap_seconds=overlap, top_k=K, model_rate=rate, events=flt, extend=cap)
    assert wav.analyze_files([path], clf, **kw) == [want]
    export = wav.ClipExport(length_seconds=20001 / rate, pre_capture_seconds=5000 / rate, extended=True, max_seconds=40 * CLIP / rate, normalize=False,
                            max_clips=int(ev.size))
    got = wav.analyze_files([path], clf, export=export, **kw)[0]
    cut = host.event_clip_spans(ev, [x.size], HOP, export.settings(rate))
    assert [t[:5] for t in got] == want and [(t[5], t[6]) for t in got] == [(int(s["start"]), int(s["length"])) for s in cut]
    assert all(t[7] is not None for t in got)
    with pytest.raises(ValueError):
        wav.analyze_files([path], clf, extend=cap)
    clf.close()


def test_window_batcher_extended_capture(gpu, tiny_cfg, tiny_blob):
    """WindowBatcher(events=, extend=, capture=) with an extended export: every class the model ranks is a hit in every window, so an
    event lasts until max_windows; its clip is cut from its first hit's pre-capture to `post` behind its LAST hit, and the FLAC
    decodes to that slice of the test's own copy of the stream."""
    from birdnet_go_amd import results as R, stream as S
    clf = host.HipClassifier(tiny_blob, device=0, max_batch=8)
    nc = clf.num_species()
    bn = host.BirdNET(clf, [f"sp{i}" for i in range(nc)], sensitivity=1.0)
    n, rate = tiny_cfg.n_samples, tiny_cfg.sample_rate
    spec = S.ModelSpec(rate, 3.0, clip_bytes=n * 2)
    overlap, hop = n // 2, n - n // 2
    thr = np.full(nc, -1.0, np.float32)
    thr[0] = np.inf
    hold = 2
    flt = host.EventTables(thr, None, 0.0, hold, 1, 0)
    ext = host.EventExtend(None, max_windows=6, short_wait=2, medium_from=2, medium_wait=2, long_from=4, long_wait=3)
    pre, post = hop // 2, 2 * hop
    export = wav.ClipExport(length_seconds=(pre + post) / rate, pre_capture_seconds=pre / rate, extended=True, max_seconds=40 * hop / rate,
                            normalize=False, lpc_order=8)
    x = export.settings(rate)
    assert (x.pre_samples, x.post_samples, x.extended) == (pre, post, True)
    rng = np.random.default_rng(23)
    n_win = 16
    t = np.arange(hop * (n_win + 1)) / rate
    streams = {f"src{i}": (np.clip(0.4 * np.sin(2 * np.pi * (600 + 400 * i) * t) + rng.normal(0, 0.05, t.size), -1, 1) * 32767).astype("<i2") for i in range(2)}
    o = S.Orchestrator()
    o.register("tiny", bn, spec)
    wb = S.WindowBatcher(o, R.ResultsQueue(size=1000), max_batch=8, events=flt, extend=ext,
                         capture=S.CaptureSettings(60 * hop / rate, export, max_sources=4))
    for s in streams:
        wb.allocate(s, "tiny")
    events = []
    step = hop // 2 + 13
    for lo in range(0, t.size, step):
        for s, x16 in streams.items():
            wb.write(s, x16[lo:lo + step].tobytes())
        wb.tick()
        events += wb.take_events()
    clips = wb.take_clips()
    assert wb.event_banks["tiny"].extended and wb.event_banks["tiny"].slots_per_source == min(min(10, nc) * 3, nc)
    long_events = [e for e in events if e["last_window"] - e["first_window"] >= hold]
    assert long_events and max(e["last_window"] - e["first_window"] for e in events) == 5       # max_windows 6: b .. b + 5
    bank = wb.capture_banks["tiny"]
    ev = np.zeros(len(events), host.EVENT)
    for i, e in enumerate(events):
        ev[i] = (int(e["source"][3:]), e["class_index"], e["first_window"], e["last_window"], e["best_window"], e["count"], e["confidence"], e["status"])
    wr, old = bank.positions()
    want, status = capref.spans(ev, wr, old, hop, pre, post, x.max_samples, True, np.full(4, -overlap, np.int64))
    key = lambda source, c, fw: (source, int(c), int(fw))
    got = {key(c["source"], c["class_index"], c["first_window"]): c for c in clips}
    done = [i for i in range(len(events)) if status[i] in (capref.OK, capref.CLAMPED)]
    assert len(got) == len(clips) == len(done) and any(status[i] == capref.OK and events[i] in long_events for i in done)
    decoded = flac.decode_clips([c["flac"] for c in clips])[0]
    for c, dec in zip(clips, decoded):
        assert np.array_equal(dec, streams[c["source"]][c["start"]:c["start"] + c["length"]])
    for i in done:
        e, c = events[i], got[key(events[i]["source"], events[i]["class_index"], events[i]["first_window"])]
        assert (c["start"], c["length"]) == (int(want[i]["start"]), int(want[i]["length"]))
        if status[i] == capref.OK:               # the test's own arithmetic: first hit's pre-capture to `post` behind the last hit
            assert c["start"] == e["first_window"] * hop - overlap - pre
            assert c["start"] + c["length"] == e["last_window"] * hop - overlap + post
    wb.close()
    clf.close()
