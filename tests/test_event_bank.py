"""The real-time event bank on the device: crafted rows, every answer np.array_equal to the streaming restatement (tests/evbankref.py)
and, once flushed, to host.detection_events over the joined rows; then the fused tick and WindowBatcher(events=...)."""
import ctypes as C

import numpy as np
import pytest

from birdnet_go_amd import host

import evbankref
import evref
from test_event_bank_ref import by_key, detection_rows, feed, filters, topk_rows

pytestmark = pytest.mark.gpu


class Pair:
    """A device bank and the restatement side by side: every entry is called on both and the answers compared."""

    def __init__(self, max_sources, n_classes, k, flt):
        self.dev = host.EventBank(n_classes, k, flt, max_sources)
        self.ref = evbankref.EventBank(max_sources, n_classes, k, flt)
        self.n_classes, self.flt = n_classes, flt
        assert self.dev.slots_per_source == self.ref.slots_per_source and self.dev.hold_windows == flt.hold_windows
        self.answers = []

    def _same(self, got, want):
        assert got.dtype == evref.EVENT and np.array_equal(got, want), (got, want)
        return got

    def process(self, sources, conf, idx):
        got = self._same(self.dev.process(sources, conf, idx), self.ref.process(sources, conf, idx))
        self.answers.append(got)
        return got

    def flush(self, source=-1):
        got = self._same(self.dev.flush(source), self.ref.flush(source))
        self.answers.append(got)
        return got

    def pending(self):
        return self._same(self.dev.pending(), self.ref.pending())

    def reset(self, source=-1):
        self.dev.reset(source)
        self.ref.reset(source)

    def set_filter(self, flt):
        self.dev.set_filter(flt)
        self.ref.set_filter(flt)
        self.flt = flt

    def clocks(self, sources):
        got = [self.dev.clock(s) for s in sources]
        assert got == [self.ref.clock(s) for s in sources]
        return got

    def flushed_is_one_shot(self, conf, idx):
        """Flushes; everything answered so far is then what bnhip_detection_events finds in the joined rows conf / idx [src, win, k]."""
        self.flush()
        assert self.pending().size == 0
        want = host.detection_events(detection_rows(conf, idx), self.n_classes, self.flt)
        assert np.array_equal(by_key(self.answers), want)
        return want

    def close(self):
        self.dev.close()


def plain_filter(n_classes, hold, min_count=1, flags=0, veto=None, thr=0.5, veto_thr=0.5):
    return host.EventTables(np.full(n_classes, thr, np.float32), veto, veto_thr, hold, min_count, flags)


# ------------------------------------------------------------------------------------------ slots
@pytest.mark.parametrize("k,hold", [(10, 6), (10, 7), (64, 64)])
def test_every_slot_live_at_once(gpu, k, hold):
    """slots_per_source 60 and 70 on both sides of a lane step, and 4096, the most: window w brings k classes of its own, so while
    window hold - 1 is applied every slot is live; the classes then come round again and open the next events in the slots just freed.
    Source 1 numbers its classes from the top."""
    n_classes, n_win = k * hold, hold + 2
    idx = np.full((2, n_win, k), -1, np.int32)
    for w in range(n_win):
        idx[0, w] = (w % hold) * k + np.arange(k)
        idx[1, w] = n_classes - 1 - ((w % hold) * k + np.arange(k))
    conf = np.full(idx.shape, 0.75, np.float32)
    conf[:, 1::2] = 0.875
    p = Pair(2, n_classes, k, plain_filter(n_classes, hold))
    assert p.dev.slots_per_source == k * hold
    feed(p, conf[:, :hold - 1], idx[:, :hold - 1], "all")                     # one call: hold - 1 windows of both sources
    assert p.pending().size == 2 * k * (hold - 1)
    for w in range(hold - 1, n_win):                                          # window hold - 1 fills the slots and frees the first k
        got = p.process([1, 0], conf[::-1, w], idx[::-1, w])
        assert got.size == 2 * k and set(got["first_window"]) == {w - hold + 1}
    p.flushed_is_one_shot(conf, idx)
    p.close()


def test_fewer_classes_than_k_times_hold(gpu):
    rng = np.random.default_rng(2)
    n_classes, k, hold = 12, 5, 4
    conf, idx = topk_rows(rng, 3, 30, n_classes, k, empty_share=0.05)
    p = Pair(3, n_classes, k, host.EventTables(np.full(n_classes, 0.1, np.float32), None, 0.0, hold, 1, 0))
    assert p.dev.slots_per_source == 12
    feed(p, conf, idx, "groups", np.random.default_rng(3))
    p.pending()
    p.flushed_is_one_shot(conf, idx)
    p.close()


# ------------------------------------------------------------------------------------------ the rule on random rows
@pytest.mark.parametrize("hold", [1, 3, 8])
@pytest.mark.parametrize("plan", ["window", "all", "groups"])
def test_random_rows(gpu, hold, plan):
    """Ties, == threshold, NaN confidences, +inf and NaN thresholds, veto classes, empty windows; min_count 1 and 3, dropped events kept
    and not; a source with 1, 2 .. hold + 2 windows in a call, sources absent from a call."""
    for min_count, flags in [(1, 0), (3, evref.KEEP_DROPPED), (3, 0)]:
        rng = np.random.default_rng(100 * hold + min_count + flags)
        n_src, n_win, n_classes, k = 4, 24, 14, 4
        conf, idx = topk_rows(rng, n_src, n_win, n_classes, k)
        p = Pair(n_src + 1, n_classes, k, filters(rng, n_classes, hold, min_count, True, flags))
        feed(p, conf, idx, plan, np.random.default_rng(hold))
        p.pending()
        assert p.clocks(range(n_src + 1)) == [n_win] * n_src + [0]
        want = p.flushed_is_one_shot(conf, idx)
        assert want.size or (min_count > 1 and not flags)
        p.close()


def test_hold_boundaries_in_one_call(gpu):
    """Hits of one class at b, b + hold - 1 and b + hold in the same call: the second joins, the third opens the next event in the
    window after the one that flushed the first; with hold_windows 1 every hit is its own event."""
    n_classes, k = 6, 2
    for hold in (1, 4):
        n_win = 2 * hold + 3
        idx = np.full((1, n_win, k), -1, np.int32)
        conf = np.zeros(idx.shape, np.float32)
        for w, x in [(1, 0.75), (hold, 0.875), (hold + 1, 0.875), (2 * hold + 1, 0.625)]:       # b = 1: joins at b + hold - 1, next at b + hold
            idx[0, w, 1], conf[0, w, 1] = 3, x
        idx[0, :, 0], conf[0, :, 0] = 5, 0.25                                                    # below the threshold throughout
        for split in (n_win, hold + 1, 1):
            p = Pair(1, n_classes, k, plain_filter(n_classes, hold))
            for w0 in range(0, n_win, split):
                p.process([0] * min(split, n_win - w0), conf[0, w0:w0 + split], idx[0, w0:w0 + split])
            want = p.flushed_is_one_shot(conf, idx)
            if hold == 4:
                assert want[["first_window", "last_window", "best_window", "count"]].tolist() == [(1, 4, 4, 2), (5, 5, 5, 1), (9, 9, 9, 1)]
            else:
                assert want["first_window"].tolist() == [1, 2, 3] and (want["count"] == 1).all()
            p.close()


def test_skipped_rows_and_empty_windows(gpu):
    """sources[r] = -1 skips a row; a row whose every idx is -1 only advances the clock; a call with no row that counts touches no device
    state."""
    n_classes, k, hold = 8, 3, 3
    p = Pair(3, n_classes, k, plain_filter(n_classes, hold))
    hit = (np.full((1, k), 0.75, np.float32), np.array([[1, -1, 2]], np.int32))
    none = (np.full((1, k), 0.75, np.float32), np.full((1, k), -1, np.int32))
    assert p.process([], np.zeros((0, k), np.float32), np.zeros((0, k), np.int32)).size == 0
    assert p.process([-1], *hit).size == 0 and p.clocks([0, 1, 2]) == [0, 0, 0]
    p.process([2, -1, 2], np.concatenate([hit[0]] * 3), np.concatenate([hit[1], hit[1], none[1]]))
    assert p.clocks([0, 1, 2]) == [0, 0, 2] and p.pending().size == 2
    got = p.process([2, 0], np.concatenate([none[0]] * 2), np.concatenate([none[1]] * 2))        # window 2 of source 2: b + hold <= w + 1
    assert got["recording"].tolist() == [2, 2] and got["count"].tolist() == [1, 1] and p.clocks([0, 2]) == [1, 3]
    p.close()


# ------------------------------------------------------------------------------------------ veto
def test_veto_windows_and_min_count_first(gpu):
    """An event at b = 3 with hold 4, and the source's veto hit at b - 1, b, b + hold - 1 or b + hold: vetoed for the two inside.  An
    event below min_count is status 1 whatever the veto says."""
    n_classes, k, hold, b = 5, 2, 4, 3
    veto = np.array([1, 0, 0, 0, 0], np.uint8)
    at = [b - 1, b, b + hold - 1, b + hold]
    n_win = b + hold + 2
    idx = np.full((4, n_win, k), -1, np.int32)
    conf = np.full(idx.shape, 0.75, np.float32)
    for s, v in enumerate(at):
        idx[s, b, 0], idx[s, b + 1, 0] = 2, 2                   # two hits: the count reaches min_count
        idx[s, b + 1, 1] = 3                                    # one hit: below it, though the veto window may cover it
        idx[s, v, 1 if v != b + 1 else 0] = 0
    assert (idx[:, b + 1, 1] == 3).all()
    for plan in ("window", "all"):
        p = Pair(4, n_classes, k, plain_filter(n_classes, hold, min_count=2, flags=evref.KEEP_DROPPED, veto=veto))
        feed(p, conf, idx, plan, np.random.default_rng(0))
        want = p.flushed_is_one_shot(conf, idx)
        assert want[want["class_index"] == 2]["status"].tolist() == [0, 2, 2, 0]
        assert want[want["class_index"] == 3]["status"].tolist() == [1, 1, 1, 1]
        p.close()


# ------------------------------------------------------------------------------------------ grid edges
def test_one_source_and_257_sources(gpu):
    """One source; 257 sources in one call (past one scan block), the rows interleaved; the last source with the last class."""
    rng = np.random.default_rng(9)
    n_classes, k, hold = 9, 3, 2
    for n_src in (1, 257):
        conf, idx = topk_rows(rng, n_src, 5, n_classes, k, empty_share=0.0)
        idx[n_src - 1, :, 0], conf[n_src - 1, :, 0] = n_classes - 1, 0.984375
        p = Pair(n_src, n_classes, k, host.EventTables(np.full(n_classes, 0.3, np.float32), None, 0.0, hold, 1, 0))
        calls = feed(p, conf, idx, "all", np.random.default_rng(n_src))
        assert len(calls) == 1 and calls[0][0].size
        want = p.flushed_is_one_shot(conf, idx)
        assert (want[-1]["recording"], want[-1]["class_index"]) == (n_src - 1, n_classes - 1)
        p.close()


# ------------------------------------------------------------------------------------------ entries and transactions
def test_pending_reset_set_filter(gpu):
    rng = np.random.default_rng(4)
    n_classes, k, hold = 10, 3, 5
    conf, idx = topk_rows(rng, 3, 12, n_classes, k, empty_share=0.0)
    flt = host.EventTables(np.full(n_classes, 0.2, np.float32), None, 0.0, hold, 1, 0)
    p = Pair(3, n_classes, k, flt)
    assert p.pending().size == 0
    feed(p, conf[:, :4], idx[:, :4], "window")
    before = p.pending()
    assert before.size and (before["status"] == host.EVENT_PENDING).all() and np.array_equal(before, p.pending())
    p.reset(1)
    after = p.pending()
    assert np.array_equal(after, before[before["recording"] != 1]) and p.clocks([0, 1, 2]) == [4, 0, 4]
    with pytest.raises(host.HipError):
        p.dev.set_filter(host.EventTables(flt.class_threshold, None, 0.0, hold + 1, 1, 0))
    assert np.array_equal(p.dev.pending(), after)
    # from the next call on: nothing hits any more, min_count 9 drops what is live, and the drops are answered
    p.set_filter(host.EventTables(np.full(n_classes, np.inf, np.float32), None, 0.0, hold, 9, evref.KEEP_DROPPED))
    feed(p, conf[:, 4:], idx[:, 4:], "groups", np.random.default_rng(1))
    assert p.pending().size == 0 and (np.concatenate(p.answers)["status"] == evref.FEW).any()
    p.reset()
    assert p.clocks([0, 1, 2]) == [0, 0, 0] and p.flush().size == 0
    p.close()


def test_failed_call_changes_nothing(gpu):
    """cap one below the need: BNHIP_E_INVALID, *n_out the need, nothing written; pending and the clocks as before; the same call with
    room then answers in full.  Process and flush alike."""
    lib = host._event_bank_protos(host.load_library())
    n_classes, k, hold = 8, 4, 2
    conf = np.full((2, 3, k), 0.75, np.float32)
    idx = np.tile(np.arange(k, dtype=np.int32), (2, 3, 1))
    idx[:, 1] += 4                                                     # window 1 opens four more; window 1 and 2 flush four each
    p = Pair(2, n_classes, k, plain_filter(n_classes, hold))
    p.process([0, 1], conf[:, 0], idx[:, 0])
    before = p.pending()
    src = np.array([0, 1, 0, 1], np.int32)
    c2, i2 = np.ascontiguousarray(conf[:, 1:].transpose(1, 0, 2)).reshape(4, k), np.ascontiguousarray(idx[:, 1:].transpose(1, 0, 2)).reshape(4, k)
    want = p.ref.process(src, c2, i2)
    assert want.size == 16
    out = np.zeros(want.size, host.EVENT)
    out["count"] = -7
    n = C.c_size_t(0)
    rc = lib.bnhip_event_bank_process(p.dev._h, src.ctypes.data, 4, c2.ctypes.data, i2.ctypes.data, out.ctypes.data, want.size - 1, C.byref(n))
    assert rc == host.E_INVALID and n.value == want.size and b"too small" in lib.bnhip_last_error() and (out["count"] == -7).all()
    assert np.array_equal(p.dev.pending(), before) and [p.dev.clock(s) for s in (0, 1)] == [1, 1]
    with pytest.raises(host.HipError) as ei:
        p.dev.process(src, c2, i2, cap=0)
    assert ei.value.needed == want.size
    assert np.array_equal(p.dev.process(src, c2, i2, cap=want.size), want) and [p.dev.clock(s) for s in (0, 1)] == [3, 3]
    p.process([0, 1], conf[:, 1], idx[:, 1])                           # window 3 opens four per source again
    live = p.pending()
    assert live.size == 8
    with pytest.raises(host.HipError) as ei:
        p.dev.flush(cap=live.size - 1)
    assert ei.value.needed == live.size and np.array_equal(p.dev.pending(), live)
    p.flush()
    # what the entries refuse of a call, the bank untouched
    for bad in (dict(sources=[2]), dict(sources=[0], idx=[[0, 1, 2, n_classes]])):
        with pytest.raises(host.HipError):
            p.dev.process(bad["sources"], np.zeros((1, k), np.float32), np.array(bad.get("idx", [[0, 1, 2, 3]]), np.int32))
    for call in (lambda: p.dev.flush(2), lambda: p.dev.reset(2), lambda: p.dev.clock(-1), lambda: p.dev.clock(2)):
        with pytest.raises(host.HipError):
            call()
    assert p.clocks([0, 1]) == [4, 4]
    p.close()


def test_same_calls_same_bytes(gpu):
    rng = np.random.default_rng(12)
    n_classes, k, hold = 20, 6, 5
    conf, idx = topk_rows(rng, 40, 12, n_classes, k)
    runs = []
    for _ in range(2):
        bank = host.EventBank(n_classes, k, filters(np.random.default_rng(1), n_classes, hold, 2, True, evref.KEEP_DROPPED), 40)
        calls = feed(bank, conf, idx, "groups", np.random.default_rng(7))
        runs.append(b"".join(c[0].tobytes() for c in calls) + bank.pending().tobytes() + bank.flush().tobytes())
        bank.close()
    assert len(runs[0]) > 32 * 40 and runs[0] == runs[1]


# ------------------------------------------------------------------------------------------ the fused tick
@pytest.mark.parametrize("n_src,model_batch", [(3, 8), (140, 256), (140, 64)], ids=["small", "one-batch", "chunks"])
def test_fused_tick(gpu, tiny_cfg, tiny_blob, n_src, model_batch):
    """bnhip_windows_predict_events on the tiny model: out_conf / out_idx are bnhip_windows_predict_topk's on a twin assembler, and the
    events are EventBank.process of those rows - through the straight path, the two-phase path and the chunked pipeline."""
    from birdnet_go_amd import stream as S
    clf = host.HipClassifier(tiny_blob, device=0, max_batch=model_batch)
    nc, k, hold, n_ticks = clf.num_species(), 5, 2, 4
    clip_bytes = tiny_cfg.n_samples * 2
    overlap, read = clip_bytes // 2, clip_bytes - clip_bytes // 2
    twins = [S.NativeWindows(overlap, read, max_batch=256) for _ in range(2)]
    rng = np.random.default_rng(n_src)
    pcm = (rng.normal(0, 0.2, (n_src, n_ticks * read // 2)).clip(-1, 1) * 32767).astype("<i2")
    for w in twins:
        for s in range(n_src):
            assert w.add_source(f"mic{s}", 2 * n_ticks * clip_bytes) == s
            w.write(s, pcm[s])
    kk = min(k, nc)
    # every class the model ranks hits: thresholds below any sigmoid output, except two classes shut out
    thr = np.full(nc, -1.0, np.float32)
    thr[:2] = np.inf
    flt = host.EventTables(thr, None, 0.0, hold, 1, 0)
    fused, fed = host.EventBank(nc, kk, flt, 256), host.EventBank(nc, kk, flt, 256)
    total = 0
    for _ in range(n_ticks):
        idxs, rows, conf, idx = twins[0].predict_topk(clf, 16, k, 0, 1.0)
        idxs2, rows2, conf2, idx2, events = clf.predict_windows_events(twins[1], fused, 16, k, 0, 1.0)
        assert idxs == idxs2 == list(range(n_src)) and np.array_equal(rows, rows2)
        assert np.array_equal(conf, conf2) and np.array_equal(idx, idx2)
        assert np.array_equal(events, fed.process(idxs, conf, idx))
        total += events.size
    assert total and np.array_equal(fused.pending(), fed.pending()) and fused.clock(n_src - 1) == n_ticks
    assert clf.predict_windows_events(twins[1], fused, 16, k, 0, 1.0)[0] == [] and fused.clock(0) == n_ticks       # nothing ready: nothing runs
    other = host.EventBank(nc, kk + 1, flt, 256)
    with pytest.raises(S.StreamError, match="results"):
        clf.predict_windows_events(twins[1], other, 16, k, 0, 1.0)
    for b in (fused, fed, other):
        b.close()
    for w in twins:
        w.close()
    clf.close()


# ------------------------------------------------------------------------------------------ WindowBatcher(events=...)
def test_window_batcher_events(gpu, tiny_cfg, tiny_blob):
    """WindowBatcher(events=tables) hands the ticks' events to take_events() and on_events, with the Results exactly as without."""
    from birdnet_go_amd import results as R, stream as S
    clf = host.HipClassifier(tiny_blob, device=0, max_batch=8)
    nc = clf.num_species()
    labels = [f"sp{i}" for i in range(nc)]
    bn = host.BirdNET(clf, labels, sensitivity=1.0)
    clip_bytes = tiny_cfg.n_samples * 2
    spec = S.ModelSpec(tiny_cfg.sample_rate, 3.0, clip_bytes=clip_bytes)
    thr = np.full(nc, -1.0, np.float32)
    thr[0] = np.inf
    flt = host.EventTables(thr, None, 0.0, 3, 2, evref.KEEP_DROPPED)
    rng = np.random.default_rng(21)
    n_src, n_win = 3, 6
    t = np.arange(tiny_cfg.n_samples // 2 * (n_win + 1)) / tiny_cfg.sample_rate
    streams = {f"src{i}": (np.clip(0.4 * np.sin(2 * np.pi * (600 + 400 * i) * t) + rng.normal(0, 0.05, t.size), -1, 1) * 32767).astype("<i2").tobytes()
               for i in range(n_src)}
    queues, taken, seen = [], None, []
    for events in (flt, None):
        o = S.Orchestrator()
        o.register("tiny", bn, spec)
        wb = S.WindowBatcher(o, R.ResultsQueue(size=1000), max_batch=8, events=events, on_events=lambda m, ev: seen.extend(ev))
        for s in streams:
            wb.allocate(s, "tiny")
        for lo in range(0, len(t) * 2, 5000):
            for s, b in streams.items():
                wb.write(s, b[lo:lo + 5000])
            wb.tick()
        while wb.tick():
            pass
        msgs = []
        while wb.queue.qsize():
            msgs.append(wb.queue.get())
        queues.append([(m.source, m.pcm_data, [(d.species, d.confidence) for d in m.results]) for m in msgs])
        if events is not None:
            taken = wb.take_events()
            assert wb.take_events() == [] and set(wb.event_banks) == {"tiny"}
            wb.remove("src1")                                       # the slot's pending detections go with the source
            assert wb.event_banks["tiny"].clock(1) == 0 and wb.event_banks["tiny"].clock(0) >= n_win
        else:
            assert wb.take_events() == [] and not wb.event_banks
        wb.close()
        assert not wb.event_banks
    assert queues[0] == queues[1] and len(queues[0]) >= n_src * n_win
    assert taken and taken == seen and {e["model_id"] for e in taken} == {"tiny"}
    # the same events from the restatement fed the Results' own rows, source by source
    ref = evbankref.EventBank(n_src, nc, min(10, nc), flt)
    want = []
    for source, _, lst in queues[0]:
        s = int(source[3:])
        conf = np.full((1, ref.k), np.nan, np.float32)
        idx = np.full((1, ref.k), -1, np.int32)
        for j, (label, c) in enumerate(lst):
            conf[0, j], idx[0, j] = c, labels.index(label)
        want += [(f"src{e['recording']}", int(e["class_index"]), int(e["first_window"]), int(e["last_window"]), int(e["best_window"]),
                  int(e["count"]), float(e["confidence"]), int(e["status"])) for e in ref.process([s], conf, idx)]
    got = [(e["source"], e["class_index"], e["first_window"], e["last_window"], e["best_window"], e["count"], e["confidence"], e["status"])
           for e in taken]
    assert sorted(got) == sorted(want) and all(e["label"] == labels[e["class_index"]] for e in taken)
    clf.close()
