"""Dynamic thresholds on the device (include/bnhip.h, "Detection events: dynamic thresholds"): a dynamic bank beside the restatement
(tests/dynref.py), and after every call the events, the change records and the thresholds() arrays compared exactly - integers
equal, floats bit for bit; then the fused tick and WindowBatcher(dynamic=...).  The refusals that need no device come first."""
import ctypes as C

import numpy as np
import pytest

from birdnet_go_amd import host

import dynref
import evbankref
import evref
import evxref
from test_event_bank_ref import feed, filters, topk_rows

F = np.float32


def same_bytes(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (got, want)


class DPair:
    """A dynamic device bank and the restatement side by side: every entry is called on both, and after every call the events, the
    call's change records and the class state are the same bytes."""

    def __init__(self, max_sources, n_classes, k, flt, dyn, ext=None):
        self.dev = host.EventBank(n_classes, k, flt, max_sources, extend=ext, dynamic=dyn)
        inner = evbankref.EventBank(max_sources, n_classes, k, flt) if ext is None else evxref.EventBank(max_sources, n_classes, k, flt, ext)
        self.ref = dynref.DynamicBank(inner, dyn)
        self.records = []
        self.check()

    def check(self):
        got, want = self.dev.threshold_changes(), self.ref.take_changes()
        assert got.dtype == host.THRESHOLD_CHANGE == dynref.CHANGE
        same_bytes(got, want)
        for g, w in zip(self.dev.thresholds(), self.ref.thresholds()):
            same_bytes(g, w)
        self.ref.changes = np.zeros(0, dynref.CHANGE)                       # (taken, as the device's list is)
        self.records.append(got)
        return got

    def set_now(self, now):
        self.dev.set_now(now)
        self.ref.set_now(now)

    def process(self, sources, conf, idx, now=None):
        if now is not None:
            self.set_now(now)
        got = self.dev.process(sources, conf, idx)
        same_bytes(got, self.ref.process(sources, conf, idx))
        self.check()
        return got

    def flush(self, source=-1, now=None):
        if now is not None:
            self.set_now(now)
        got = self.dev.flush(source)
        same_bytes(got, self.ref.flush(source))
        self.check()
        return got

    def hit(self, now, x, c=0, source=0):
        """one row of one result (k 1)"""
        return self.process([source], np.array([[x]], np.float32), np.array([[c]], np.int32), now)

    def state(self, c=0):
        level, count, expires, learned_at, current = self.dev.thresholds()
        return int(level[c]), int(count[c]), int(expires[c]), int(learned_at[c]), current[c]

    def reasons(self):
        r = np.concatenate(self.records)
        return set(r["reason"].tolist())

    def close(self):
        self.dev.close()


def one_class_pair(base, trigger=0.9, min_threshold=0.1, valid=100, cooldown=10, class_dynamic=None, veto=None, n_sources=2):
    """k 1, hold 1, min_count 1: a hit is an approved event in the call that brings it."""
    base = np.asarray(base, np.float32)
    flt = host.EventTables(base, veto, 0.5, 1, 1, 0)
    return DPair(n_sources, base.size, 1, flt, host.EventDynamic(class_dynamic, trigger, min_threshold, valid, cooldown))


def random_run(p, rng, n_src, n_classes, k, n_calls, now=0):
    """Random rows of random sources at times that step by 0..3: with a valid of a few units and a small cooldown the classes learn,
    are kept alive and expire."""
    for _ in range(n_calls):
        now += int(rng.integers(0, 4))
        src = np.repeat(np.arange(n_src), rng.integers(0, 3, n_src))
        if n_src > 8:                                                       # (the scan cases: every source in every call)
            src = np.arange(n_src)
        src = src[np.argsort(rng.random(src.size), kind="stable")].astype(np.int32)
        conf = (rng.integers(0, 64, (src.size, k)) / 64.0).astype(np.float32)
        idx = np.stack([rng.permutation(max(n_classes, k))[:k] for _ in range(src.size)]).astype(np.int32).reshape(src.size, k) if src.size else np.zeros((0, k), np.int32)
        idx[idx >= n_classes] = -1
        p.process(src, conf, idx, now)
    p.flush(now=now + 1)


# ------------------------------------------------------------------------------------------ no device
def test_refusals_without_a_device(built_lib):
    lib = host._event_bank_protos(host.load_library())
    thr = np.full(8, 0.5, np.float32)
    fs = host._EventFilterStruct(thr.ctypes.data, None, 0.5, 5, 1, 0)
    h = C.c_void_p()

    def create(dyn=True, out=C.byref(h), **kw):
        d = dict(class_dynamic=None, trigger=0.9, min_threshold=0.1, valid=10, cooldown=0)
        d.update(kw)
        ds = host._EventDynamicStruct(d["class_dynamic"], d["trigger"], d["min_threshold"], d["valid"], d["cooldown"])
        return lib.bnhip_event_bank_create_dynamic(0, 4, 8, 3, C.addressof(fs), None, C.addressof(ds) if dyn else None, out)

    for kw, text in [(dict(dyn=False), b"NULL"), (dict(trigger=float("nan")), b"trigger"), (dict(trigger=-0.5), b"trigger"),
                     (dict(min_threshold=float("nan")), b"min_threshold"), (dict(min_threshold=-1.0), b"min_threshold"),
                     (dict(valid=0), b"valid"), (dict(valid=2 ** 61 + 1), b"valid"), (dict(cooldown=-1), b"cooldown"),
                     (dict(cooldown=2 ** 61 + 1), b"cooldown"), (dict(out=None), b"NULL")]:
        h.value = 12345
        assert create(**kw) == host.E_INVALID, kw
        assert text in lib.bnhip_last_error(), (kw, lib.bnhip_last_error())
        assert "out" in kw or h.value is None, kw
    n = C.c_size_t(7)
    for rc in (lib.bnhip_event_bank_set_dynamic(None, None), lib.bnhip_event_bank_set_now(None, 0),
               lib.bnhip_event_bank_threshold_changes(None, None, 0, C.byref(n)), lib.bnhip_event_bank_thresholds(None, None, None, None, None, None),
               lib.bnhip_event_bank_set_thresholds(None, None, None, None, None), lib.bnhip_event_bank_reset_thresholds(None, -1)):
        assert rc == host.E_INVALID and b"NULL" in lib.bnhip_last_error()
    assert n.value == 7
    # the one function of step 2, against the restatement: levels, the clamp, NaN and +inf, an unknown level
    for base in (0.8, 0.05, 0.3, np.inf, 1e-30):
        for level in range(4):
            for lo in (0.0, 0.1, 0.9):
                assert host.event_threshold(base, level, lo).tobytes() == dynref.threshold(base, level, lo).tobytes(), (base, level, lo)
    assert all(np.isnan(host.event_threshold(np.nan, lv, 0.1)) for lv in range(4))
    assert np.isnan(host.event_threshold(0.5, 4, 0.1)) and np.isnan(host.event_threshold(0.5, -1, 0.1))


def test_batcher_reads_its_clock_at_creation_only_with_dynamic():
    from birdnet_go_amd import stream as S
    calls = []

    def clock():
        calls.append(1)
        return 5.0

    flt = host.EventTables(np.full(4, 0.5, np.float32), None, 0.0, 1, 1, 0)
    S.WindowBatcher(S.Orchestrator(), clock=clock, events=flt).close()
    assert not calls
    wb = S.WindowBatcher(S.Orchestrator(), clock=clock, events=flt, dynamic=host.EventDynamic(None, 0.9, 0.1, 10, 0))
    assert len(calls) == 1 and wb.created == 5.0 and wb.take_threshold_changes() == []
    wb.close()
    with pytest.raises(S.StreamError, match="dynamic needs events"):
        S.WindowBatcher(S.Orchestrator(), dynamic=host.EventDynamic(None, 0.9, 0.1, 10, 0))


# ------------------------------------------------------------------------------------------ the per-class passes
@pytest.mark.gpu
@pytest.mark.parametrize("n_classes", [1, 255, 256, 257])
def test_class_counts_round_a_block(gpu, n_classes):
    """One class, and one below, at and above a block of the per-class passes; the last class learns and expires."""
    rng = np.random.default_rng(n_classes)
    k = min(4, n_classes)
    thr = (rng.integers(16, 40, n_classes) / 64.0).astype(np.float32)
    p = DPair(3, n_classes, k, host.EventTables(thr, None, 0.0, 2, 1, 0), host.EventDynamic(None, 0.7, 0.2, 6, 2))
    top = np.full((1, k), -1, np.int32)
    top[0, 0] = n_classes - 1
    for now in (0, 1):                                                      # hold 2: due, approved and learnt in the second call
        p.process([2], np.full((1, k), 0.96875, np.float32), top, now)
    assert p.state(n_classes - 1)[:2] == (1, 1)
    random_run(p, rng, 3, n_classes, k, 24, now=1)
    p.flush(now=1000)                                                       # (whatever still stands expires here)
    assert p.reasons() == {dynref.EXPIRY, dynref.HIGH_CONFIDENCE} and not p.dev.thresholds()[0].any()
    p.close()


@pytest.mark.gpu
def test_most_classes(gpu):
    """38 400 classes: the last learns and class 0 expires in one call; two records, classes ascending."""
    n_classes, k = 38400, 2
    p = DPair(1, n_classes, k, host.EventTables(np.full(n_classes, 0.5, np.float32), None, 0.0, 1, 1, 0), host.EventDynamic(None, 0.7, 0.2, 6, 0))
    state = [np.zeros(n_classes, np.int32), np.zeros(n_classes, np.int32), np.zeros(n_classes, np.int64), np.full(n_classes, -1, np.int64)]
    state[0][0], state[1][0], state[2][0], state[3][0] = 2, 2, 5, 1
    p.dev.restore_thresholds(*state)
    p.ref.restore_thresholds(*state)
    p.check()
    p.process([0], np.array([[0.9375, 0.25]], np.float32), np.array([[n_classes - 1, 0]], np.int32), now=10)
    assert p.records[-1][["class_index", "previous_level", "new_level", "reason"]].tolist() == [(0, 2, 0, dynref.EXPIRY),
                                                                                                (n_classes - 1, 0, 1, dynref.HIGH_CONFIDENCE)]
    p.close()


@pytest.mark.gpu
def test_more_records_than_come_down_with_the_count(gpu):
    """40 classes learn in one call and expire in one call: past the records that ride in the first copy back."""
    n_classes, k = 48, 40
    p = DPair(1, n_classes, k, host.EventTables(np.full(n_classes, 0.5, np.float32), None, 0.0, 1, 1, 0), host.EventDynamic(None, 0.7, 0.2, 6, 0))
    conf = (0.75 + np.arange(k) / 256.0).astype(np.float32).reshape(1, k)
    p.process([0], conf, np.arange(3, 3 + k, dtype=np.int32).reshape(1, k), now=0)
    assert p.records[-1].size == 40 and (p.records[-1]["reason"] == dynref.HIGH_CONFIDENCE).all()
    p.process([0], conf, np.full((1, k), -1, np.int32), now=7)
    assert p.records[-1].size == 40 and (p.records[-1]["reason"] == dynref.EXPIRY).all() and (np.diff(p.records[-1]["class_index"]) == 1).all()
    p.close()


# ------------------------------------------------------------------------------------------ the scan's carry, the groups
@pytest.mark.gpu
@pytest.mark.parametrize("n_src", [1, 3, 300])
def test_sources(gpu, n_src):
    """1, 3 and 300 sources (more than one 256-wide round of the scan) over 8 classes, k 3, hold 2: many sources approve a class in
    one call, and it learns once."""
    rng = np.random.default_rng(n_src)
    n_classes, k = 8, 3
    thr = np.array([0.5, 0.25, 0.625, 0.375, 0.5, np.inf, 0.4375, 0.5], np.float32)
    p = DPair(n_src, n_classes, k, host.EventTables(thr, None, 0.0, 2, 1, 0), host.EventDynamic(None, 0.75, 0.125, 5, 2))
    random_run(p, rng, n_src, n_classes, k, 10 if n_src > 8 else 40)
    assert dynref.HIGH_CONFIDENCE in p.reasons() and max(r.size for r in p.records) <= 2 * n_classes
    p.close()


# ------------------------------------------------------------------------------------------ the marking pass over a long stage
@pytest.mark.gpu
def test_long_stage(gpu):
    """One source, 400 classes, k 64, hold 5: 320 slots, every one live while window 4 is applied.  Ten windows in one call stage 384
    events - more than one block-stride of the marking pass - and the flush the 256 that are left; the approved classes and their
    largest confidences are the restatement's."""
    n_classes, k, hold, n_win = 400, 64, 5, 10
    idx = np.stack([((w % 6) * 64 + np.arange(k)) % n_classes for w in range(n_win)]).astype(np.int32)
    conf = np.array([[0.5 + ((w * 7 + j * 3) % 50) / 100.0 for j in range(k)] for w in range(n_win)], np.float32)
    p = DPair(1, n_classes, k, host.EventTables(np.full(n_classes, 0.4, np.float32), None, 0.0, hold, 1, 0), host.EventDynamic(None, 0.8, 0.05, 50, 0))
    assert p.dev.slots_per_source == 320
    got = p.process([0] * n_win, conf, idx, now=1)
    assert got.size == 384 and (p.records[-1]["reason"] == dynref.HIGH_CONFIDENCE).all() and p.records[-1].size > 64
    assert p.flush(now=2).size == 256 and p.records[-1].size > 64
    p.close()


# ------------------------------------------------------------------------------------------ the rule's edges
@pytest.mark.gpu
def test_rule_edges(gpu):
    """The restatement's literal cases (tests/test_event_dynamic_ref.py) on the device."""
    p = one_class_pair([0.8], cooldown=10)                                  # the cooldown pair
    p.hit(5, 0.95)
    assert p.hit(14, 0.95).size == 1 and p.state()[:4] == (1, 1, 114, 5)
    assert p.hit(15, 0.95).size == 1 and p.state() == (2, 2, 115, 15, F(0.4))
    p.hit(25, 0.95)
    p.hit(35, 0.95)
    assert p.state() == (3, 4, 135, 35, F(0.2)) and p.records[-1].size == 0
    p.close()
    p = one_class_pair([0.8], valid=100, cooldown=0)                        # the expiry pair, then expiry and a new learning in one call
    p.hit(0, 0.95)
    assert p.hit(100, 0.7).size == 1 and p.state()[:4] == (1, 1, 100, 0)
    assert p.hit(101, 0.7).size == 0 and p.state() == (0, 0, 100, -1, F(0.8))
    assert p.records[-1].tolist() == [(0, 1, 0, dynref.EXPIRY, F(0.6), F(0.8), 0.0, 0)]
    p.hit(101, 0.95)
    assert p.hit(150, 0.85).size == 1 and p.state()[:4] == (1, 1, 250, 101)                   # a touch
    p.hit(251, 0.95)
    assert [tuple(r)[:4] for r in p.records[-1].tolist()] == [(0, 1, 0, dynref.EXPIRY), (0, 0, 1, dynref.HIGH_CONFIDENCE)]
    p.close()
    p = one_class_pair([0.8], min_threshold=0.3, cooldown=0)                # min above base * mult
    assert [p.hit(t, 0.95).size and p.state()[4] for t in (0, 1, 2)] == [F(0.6), F(0.4), F(0.3)]
    p.close()
    p = one_class_pair([0.5], trigger=0.6, min_threshold=0.7, cooldown=0, valid=10)           # min above the base: thr_eff > base
    p.hit(0, 0.65)
    assert p.state()[4] == F(0.7) and p.hit(1, 0.69).size == 0 and p.state()[2] == 10         # above the base, not above thr_eff: no touch
    assert p.hit(2, 0.71).size == 1 and p.state()[2] == 12
    p.close()
    p = one_class_pair([0.95], trigger=0.9, cooldown=0)                     # approved under the lowered threshold with x < base
    assert p.hit(0, 0.95).size == 0 and p.hit(1, 0.96).size == 1 and p.state()[:4] == (1, 1, 101, 1)
    assert p.hit(5, 0.92).size == 1 and p.state()[:4] == (1, 1, 101, 1)                       # neither learns nor touches
    assert p.hit(7, 0.95).size == 1 and p.state()[:4] == (2, 2, 107, 7)                       # x == base learns
    p.close()
    p = one_class_pair([0.8], trigger=0.9)                                  # x == trigger does not
    assert p.hit(0, 0.9).size == 1 and p.state() == (0, 0, 0, -1, F(0.8))
    p.close()


@pytest.mark.gpu
def test_veto_nan_inf_and_custom_classes(gpu):
    """A veto class never learns or touches; NaN and +inf bases stay shut at every level; a class that is not dynamic keeps its base
    and its state."""
    base = np.array([0.5, 0.5, np.nan, np.inf, 0.5], np.float32)
    p = one_class_pair(base, trigger=0.6, cooldown=0, valid=10, veto=np.array([0, 1, 0, 0, 0], np.uint8), class_dynamic=np.array([1, 1, 1, 1, 0], np.uint8))
    state = [np.array(a) for a in ([1, 1, 2, 3, 2], [1, 1, 2, 3, 2], [50, 50, 50, 50, 5], [0, 0, 0, 0, 0])]
    p.dev.restore_thresholds(*state)
    p.ref.restore_thresholds(*state)
    p.check()
    cur = p.dev.thresholds()[4]
    assert cur[0] == F(0.375) and np.isnan(cur[2]) and cur[3] == np.inf and cur[4] == F(0.5)
    for c, events in [(1, 0), (2, 0), (3, 0), (4, 1), (0, 1)]:
        assert p.hit(20, 0.99, c=c).size == events
    assert p.state(1)[:4] == (1, 1, 50, 0) and p.state(4)[:4] == (2, 2, 5, 0) and p.state(0)[:4] == (2, 2, 30, 20)
    p.close()


# ------------------------------------------------------------------------------------------ the transaction
@pytest.mark.gpu
def test_a_refused_call_changes_no_class(gpu):
    lib = host._event_bank_protos(host.load_library())
    p, twin = one_class_pair([0.8, 0.8], cooldown=0), one_class_pair([0.8, 0.8], cooldown=0)
    for q in (p, twin):
        q.hit(0, 0.95)
    before = [a.copy() for a in p.dev.thresholds()]
    row = ([0], np.array([[0.95]], np.float32), np.array([[0]], np.int32))
    p.set_now(500)
    with pytest.raises(host.HipError) as ei:
        p.dev.process(*row, cap=0)
    assert ei.value.needed == 1
    for g, w in zip(p.dev.thresholds(), before):
        same_bytes(g, w)
    out, n = np.zeros(4, host.THRESHOLD_CHANGE), C.c_size_t(0)
    assert lib.bnhip_event_bank_threshold_changes(p.dev._h, out.ctypes.data, 4, C.byref(n)) == 0 and n.value == 1      # the first call's, still
    same_bytes(out[:1], p.records[-1])
    assert lib.bnhip_event_bank_threshold_changes(p.dev._h, out.ctypes.data, 0, C.byref(n)) == host.E_INVALID and n.value == 1
    for q in (p, twin):                                                     # the repeat with room is the run that never failed
        q.process(*row, now=500)
    same_bytes(p.records[-1], twin.records[-1])
    assert p.records[-1].size == 2 and p.state()[:4] == twin.state()[:4] == (1, 1, 600, 500)
    flt = host.EventTables(np.array([0.8], np.float32), None, 0.0, 4, 1, 0)     # pending changes nothing; flush learns
    q = DPair(1, 1, 1, flt, host.EventDynamic(None, 0.9, 0.1, 100, 0))
    assert q.hit(3, 0.95).size == 0
    same_bytes(q.dev.pending(), q.ref.pending())
    q.check()
    assert q.state()[:4] == (0, 0, 0, -1) and q.flush(now=9).size == 1 and q.state()[:4] == (1, 1, 109, 9)
    assert q.hit(10, 0.95).size == 0 and q.state()[:4] == (1, 1, 110, 9)    # (a touch; the event is live)
    q.set_now(20)
    with pytest.raises(host.HipError):                                      # the flush refused for room changes no class either
        q.dev.flush(cap=0)
    assert q.state()[:4] == (1, 1, 110, 9) and q.flush().size == 1 and q.state()[:4] == (2, 2, 120, 20)
    for b in (p, twin, q):
        b.close()


@pytest.mark.gpu
def test_pending_does_not_repeat_the_records(gpu):
    """pending changes nothing: the records of the call before it still stand in the library, and threshold_changes() hands each
    of them out once."""
    lib = host._event_bank_protos(host.load_library())
    flt = host.EventTables(np.array([0.8], np.float32), None, 0.0, 1, 1, 0)
    bank = host.EventBank(1, 1, flt, 2, dynamic=host.EventDynamic(None, 0.9, 0.1, 100, 0))
    row = ([0], np.array([[0.95]], np.float32), np.array([[0]], np.int32))
    bank.set_now(1)
    assert bank.process(*row).size == 1
    assert bank.pending().size == 0 and bank.pending().size == 0
    got = bank.threshold_changes()
    assert got[["class_index", "previous_level", "new_level", "reason"]].tolist() == [(0, 0, 1, host.THRESHOLD_HIGH_CONFIDENCE)]
    assert bank.pending().size == 0 and bank.threshold_changes().size == 0
    out, n = np.zeros(4, host.THRESHOLD_CHANGE), C.c_size_t(0)                  # (the library's list: the last process call's, still)
    assert lib.bnhip_event_bank_threshold_changes(bank._h, out.ctypes.data, 4, C.byref(n)) == 0 and n.value == 1
    same_bytes(out[:1], got)
    bank.set_now(2)
    assert bank.process(*row).size == 1 and bank.pending().size == 0            # a second learning, then pending again
    assert bank.threshold_changes()[["previous_level", "new_level"]].tolist() == [(1, 2)]
    bank.close()


# ------------------------------------------------------------------------------------------ the surface
@pytest.mark.gpu
def test_surface(gpu):
    rng = np.random.default_rng(3)
    n = 300
    base = (rng.integers(16, 48, n) / 64.0).astype(np.float32)
    p = DPair(2, n, 2, host.EventTables(base, None, 0.0, 1, 1, 0), host.EventDynamic(None, 0.7, 0.2, 50, 0))
    count = rng.integers(0, 6, n).astype(np.int32)
    state = [np.minimum(count, 3).astype(np.int32), count, rng.integers(0, 2 ** 62, n), rng.integers(-1, 2 ** 62, n)]
    p.dev.restore_thresholds(*state)                                        # the round trip
    p.ref.restore_thresholds(*state)
    for g, w in zip(p.dev.thresholds()[:4], state):
        assert np.array_equal(g, w)
    p.check()
    for bad in ([4, 4, 0, 0], [-1, 0, 0, 0], [2, 3, 0, 0], [3, 2, 0, 0], [1, 1, -1, 0], [1, 1, 0, -2]):
        worse = [a.copy() for a in state]
        for a, v in zip(worse, bad):
            a[n - 1] = v
        with pytest.raises(host.HipError):
            p.dev.restore_thresholds(*worse)
    with pytest.raises(host.HipError):
        p.dev.restore_thresholds(*[a[:-1] for a in state])
    p.check()                                                               # (refused: nothing moved)
    for c in (7, n - 1):
        p.dev.reset_thresholds(c)
        p.ref.reset_thresholds(c)
        p.check()
        assert p.state(c)[:4] == (0, 0, 0, -1)
    for c in (n, -2):
        with pytest.raises(host.HipError):
            p.dev.reset_thresholds(c)
    p.dev.reset_thresholds()
    p.ref.reset_thresholds()
    p.check()
    assert not p.dev.thresholds()[1].any()
    # set_filter with new bases: the next call's thresholds follow them
    rows = (np.array([0, 1], np.int32), np.array([[0.96875, 0.1], [0.96875, 0.1]], np.float32), np.array([[5, 6], [9, 6]], np.int32))
    p.process(*rows, now=1)
    assert p.state(5)[0] == 1 and p.state(5)[4] == dynref.threshold(base[5], 1, 0.2)
    flt2 = host.EventTables((base / 2).astype(np.float32), None, 0.0, 1, 1, 0)
    p.dev.set_filter(flt2)
    p.ref.set_filter(flt2)
    p.process(*rows, now=2)
    assert p.state(5)[0] == 2 and p.state(5)[4] == dynref.threshold(base[5] / 2, 2, 0.2)
    # set_dynamic(None) freezes: thr_eff = base, the state stays, nothing is learnt; a new dynamic takes it up again
    p.dev.set_dynamic(None)
    p.ref.set_dynamic(None)
    frozen = [a.copy() for a in p.dev.thresholds()[:4]]
    p.process(*rows, now=3)
    p.flush(now=10 ** 6)
    for g, w in zip(p.dev.thresholds()[:4], frozen):
        assert np.array_equal(g, w)
    assert np.array_equal(p.dev.thresholds()[4], flt2.class_threshold)
    dyn2 = host.EventDynamic(None, 0.9, 0.01, 5, 0)
    p.dev.set_dynamic(dyn2)
    p.ref.set_dynamic(dyn2)
    p.process(*rows, now=10 ** 6 + 1)
    assert p.records[-1].size >= 2 and dynref.EXPIRY in p.reasons()
    # bank time never decreases
    for bad in (10 ** 6, -1, 2 ** 62):
        with pytest.raises(host.HipError):
            p.dev.set_now(bad)
    p.set_now(2 ** 62 - 1)
    p.close()
    # the entries of a dynamic bank on a plain one
    plain = host.EventBank(n, 2, flt2, 2)
    for call in (lambda: plain.set_now(1), lambda: plain.set_dynamic(None), lambda: plain.set_dynamic(dyn2), plain.thresholds, plain.reset_thresholds,
                 lambda: plain.restore_thresholds(*state), plain._collect_changes):
        with pytest.raises(host.HipError, match="without a dynamic"):
            call()
    plain.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hold", [1, 3, 8])
def test_no_dynamic_class_answers_the_plain_bank(gpu, hold):
    """class_dynamic all zero: the plain bank's events byte for byte over test_event_bank_ref's random rows."""
    rng = np.random.default_rng(100 * hold)
    n_src, n_win, n_classes, k = 4, 24, 14, 4
    conf, idx = topk_rows(rng, n_src, n_win, n_classes, k)
    flt = filters(rng, n_classes, hold, 3, True, evref.KEEP_DROPPED)
    plain = host.EventBank(n_classes, k, flt, n_src)
    quiet = host.EventBank(n_classes, k, flt, n_src, dynamic=host.EventDynamic(np.zeros(n_classes, np.uint8), 0.1, 0.05, 3, 0))
    a = feed(plain, conf, idx, "groups", np.random.default_rng(hold))
    quiet.set_now(5)
    b = feed(quiet, conf, idx, "groups", np.random.default_rng(hold))
    assert len(a) == len(b) and sum(x[0].size for x in a) > 0
    for x, y in zip(a, b):
        same_bytes(x[0], y[0])
    same_bytes(plain.pending(), quiet.pending())
    same_bytes(plain.flush(), quiet.flush())
    assert quiet.threshold_changes().size == 0 and not quiet.thresholds()[1].any()
    plain.close()
    quiet.close()


# ------------------------------------------------------------------------------------------ extended + dynamic
@pytest.mark.gpu
def test_extended_and_dynamic(gpu):
    rng = np.random.default_rng(77)
    n_src, n_classes, k, hold = 3, 10, 3, 2
    ext = host.EventExtend(np.array([1, 0] * 5, np.uint8), 8, 3, 2, 2, 4, 1)
    thr = (rng.integers(16, 40, n_classes) / 64.0).astype(np.float32)
    p = DPair(n_src, n_classes, k, host.EventTables(thr, None, 0.0, hold, 1, 0), host.EventDynamic(None, 0.7, 0.125, 6, 2), ext)
    assert p.dev.slots_per_source == p.ref.inner.slots_per_source == 9
    random_run(p, rng, n_src, n_classes, k, 60)
    assert p.reasons() == {dynref.EXPIRY, dynref.HIGH_CONFIDENCE}
    p.close()


# ------------------------------------------------------------------------------------------ the fused tick
@pytest.mark.gpu
def test_fused_tick(gpu, tiny_cfg, tiny_blob):
    """bnhip_windows_predict_events with a dynamic bank is predict_topk's rows fed to a dynamic twin, tick by tick: the events, the
    change records and the class state."""
    from birdnet_go_amd import stream as S
    clf = host.HipClassifier(tiny_blob, device=0, max_batch=8)
    nc, k, hold, n_ticks, n_src = clf.num_species(), 5, 1, 5, 3
    clip_bytes = tiny_cfg.n_samples * 2
    overlap, read = clip_bytes // 2, clip_bytes - clip_bytes // 2
    twins = [S.NativeWindows(overlap, read, max_batch=256) for _ in range(2)]
    rng = np.random.default_rng(5)
    pcm = (rng.normal(0, 0.2, (n_src, n_ticks * read // 2)).clip(-1, 1) * 32767).astype("<i2")
    for w in twins:
        for s in range(n_src):
            assert w.add_source(f"mic{s}", 2 * n_ticks * clip_bytes) == s
            w.write(s, pcm[s])
    kk = min(k, nc)
    flt = host.EventTables(np.full(nc, 1e-6, np.float32), None, 0.0, hold, 1, 0)
    dyn = host.EventDynamic(None, 1e-6, 0.0, 15, 10)                         # whatever the model ranks is approved high
    fused, fed = host.EventBank(nc, kk, flt, 256, dynamic=dyn), host.EventBank(nc, kk, flt, 256, dynamic=dyn)
    records = 0
    for t in range(n_ticks):
        for b in (fused, fed):
            b.set_now(10 * t)
        idxs, rows, conf, idx = twins[0].predict_topk(clf, 16, k, 0, 1.0)
        idxs2, rows2, conf2, idx2, events = clf.predict_windows_events(twins[1], fused, 16, k, 0, 1.0)
        assert idxs == idxs2 == list(range(n_src)) and np.array_equal(conf, conf2) and np.array_equal(idx, idx2)
        same_bytes(events, fed.process(idxs, conf, idx))
        got = fused.threshold_changes()
        same_bytes(got, fed.threshold_changes())
        records += got.size
        for g, w in zip(fused.thresholds(), fed.thresholds()):
            same_bytes(g, w)
    assert records and fused.thresholds()[0].max() == 3
    assert clf.predict_windows_events(twins[1], fused, 16, k, 0, 1.0)[0] == [] and fused.threshold_changes().size == 0     # nothing ready: no call
    for b in (fused, fed):
        b.close()
    for w in twins:
        w.close()
    clf.close()


# ------------------------------------------------------------------------------------------ WindowBatcher(dynamic=...)
@pytest.mark.gpu
def test_window_batcher_dynamic(gpu, tiny_cfg, tiny_blob):
    """A species repeated above the trigger lowers its threshold, and a quieter call of it is then detected, which the same batcher
    without `dynamic` misses.  Two tones stand for the loud and the quiet call: a probe run finds the species whose confidences under
    the two lie furthest apart, and its threshold is put between them.  The events of both runs are the restatements' over the
    Results' own rows."""
    from birdnet_go_amd import results as R, stream as S
    clf = host.HipClassifier(tiny_blob, device=0, max_batch=8)
    nc = clf.num_species()
    labels = [f"sp{i}" for i in range(nc)]
    bn = host.BirdNET(clf, labels, sensitivity=1.0)
    clip_bytes = tiny_cfg.n_samples * 2
    spec = S.ModelSpec(tiny_cfg.sample_rate, 3.0, clip_bytes=clip_bytes)
    n_win = 6
    t = np.arange(tiny_cfg.n_samples // 2 * (n_win + 1)) / tiny_cfg.sample_rate
    tone = {f: (0.4 * np.sin(2 * np.pi * f * t) * 32767).astype("<i2").tobytes() for f in (700.0, 2300.0)}
    kk = min(10, nc)

    def run(streams, **kw):
        """-> the batcher's Results as per-source rows [(conf [kk], idx [kk])], its events, its threshold changes (taken, seen)"""
        now = [100.0]
        o = S.Orchestrator()
        o.register("tiny", bn, spec)
        seen = []
        wb = S.WindowBatcher(o, R.ResultsQueue(size=1000), max_batch=8, clock=lambda: now[0],
                             on_threshold_changes=(lambda m, ch: seen.extend(ch)) if "dynamic" in kw else None, **kw)
        for s in streams:
            wb.allocate(s, "tiny")
        for lo in range(0, max(len(b) for b in streams.values()), 5000):
            for s, b in streams.items():
                wb.write(s, b[lo:lo + 5000])
            now[0] += 1.0
            wb.tick()
        now[0] += 1.0
        while wb.tick():
            now[0] += 1.0
        rows = {s: [] for s in streams}
        while wb.queue.qsize():
            m = wb.queue.get()
            conf, idx = np.full(kk, np.nan, np.float32), np.full(kk, -1, np.int32)
            for j, d in enumerate(m.results):
                conf[j], idx[j] = d.confidence, labels.index(d.species)
            rows[m.source].append((conf, idx))
        events, taken = wb.take_events(), wb.take_threshold_changes()
        wb.close()
        return rows, events, taken, seen

    probe, _, _, _ = run({str(f): b for f, b in tone.items()})
    per = {f: np.full((len(probe[f]), nc), np.nan) for f in probe}                  # [window, class] confidences of each tone
    for f, lst in probe.items():
        for w, (conf, idx) in enumerate(lst):
            per[f][w, idx[idx >= 0]] = conf[idx >= 0]
    a, b = per["700.0"], per["2300.0"]
    gaps = {(c, hi): (x.min(0)[c] - y.max(0)[c]) for hi, (x, y) in {"700.0": (a, b), "2300.0": (b, a)}.items() for c in range(nc)
            if not np.isnan(x[:, c]).any() and not np.isnan(y[:, c]).any()}
    (c, loud), gap = max(gaps.items(), key=lambda kv: kv[1])
    quiet = "2300.0" if loud == "700.0" else "700.0"
    lo, hi = per[quiet][:, c].max(), per[loud][:, c].min()
    assert gap > 0 and per[quiet][:, c].min() > 0.25 * hi, (gap, lo, hi)            # (the tones tell the species apart; level 3 reaches the quiet one)
    thr = np.full(nc, np.inf, np.float32)
    thr[c] = np.float32((lo + hi) / 2)
    flt = host.EventTables(thr, None, 0.0, 1, 1, 0)
    dyn = host.EventDynamic(None, float(thr[c]), 0.0, 10 ** 9, 0)
    stream = {"mic": tone[float(loud)] + tone[float(quiet)]}
    out = {}
    for name, kw in (("plain", dict(events=flt)), ("dynamic", dict(events=flt, dynamic=dyn))):
        rows, events, taken, seen = run(stream, **kw)
        ref = evbankref.EventBank(1, nc, kk, flt)
        ref = dynref.DynamicBank(ref, dyn if name == "dynamic" else None)
        want = []
        for i, (conf, idx) in enumerate(rows["mic"]):
            ref.set_now(i)
            want += [(int(e["class_index"]), int(e["first_window"]), float(e["confidence"]), int(e["status"])) for e in ref.process([0], conf[None], idx[None])]
        got = [(e["class_index"], e["first_window"], e["confidence"], e["status"]) for e in events]
        assert got == want and all(e["source"] == "mic" and e["label"] == labels[c] for e in events)
        out[name] = ({e["first_window"] for e in events}, rows["mic"], taken, seen)
    plain, rows, _, _ = out["plain"]
    learnt, rows2, taken, seen = out["dynamic"]
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(rows, rows2)) and len(rows) == len(rows2)
    missed = learnt - plain
    assert plain and missed and min(missed) > min(plain)                             # heard only once the threshold had come down
    assert not out["plain"][2] and taken and taken == seen
    first = taken[0]
    assert (first["model_id"], first["class_index"], first["label"], first["previous_level"], first["new_level"], first["reason"]) == (
        "tiny", c, labels[c], 0, 1, host.THRESHOLD_HIGH_CONFIDENCE)
    assert first["previous_value"] == float(thr[c]) and first["new_value"] == float(dynref.threshold(thr[c], 1, 0.0))
    clf.close()
