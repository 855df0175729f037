"""Dynamic thresholds without a device or the library: the restatement (tests/dynref.py) pinned to a literal table of the
reference's cases (internal/analysis/processor/dynamic_threshold.go), to the plain streaming rule where no class learns, and to
itself under both walks of two sources that approve one class in one call."""
import numpy as np
import pytest

from birdnet_go_amd import host

import dynref
import evbankref
from dynref import EXPIRY, HIGH_CONFIDENCE
from test_event_bank_ref import feed, filters, topk_rows

F = np.float32


def bank(base, trigger=0.9, min_threshold=0.1, valid=100, cooldown=10, class_dynamic=None, n_sources=2, k=1, hold=1):
    """hold 1, min_count 1: a hit is an approved event in the call that brings it."""
    base = np.asarray(base, np.float32)
    flt = host.EventTables(base, None, 0.0, hold, 1, 0)
    return dynref.DynamicBank(evbankref.EventBank(n_sources, base.size, k, flt), host.EventDynamic(class_dynamic, trigger, min_threshold, valid, cooldown))


def hit(b, now, x, c=0, source=0):
    b.set_now(now)
    return b.process([source], np.array([[x]], np.float32), np.array([[c]], np.int32))


def state(b, c=0):
    level, count, expires, learned_at, current = b.thresholds()
    return int(level[c]), int(count[c]), int(expires[c]), int(learned_at[c]), current[c]


def records(b):
    return [tuple(r)[:7] for r in b.take_changes().tolist()]


def test_levels_of_a_base_of_0_8():
    """0.8 -> 0.6 -> 0.4 -> 0.2, one learning per cooldown; a fourth learning counts and stays at level 3."""
    b = bank([0.8])
    assert state(b) == (0, 0, 0, -1, F(0.8))
    want = [(0, 1, F(0.6)), (10, 2, F(0.4)), (20, 3, F(0.2)), (30, 3, F(0.2))]
    before = F(0.8)
    for i, (now, level, value) in enumerate(want):
        assert hit(b, now, 0.95).size == 1
        assert state(b) == (level, i + 1, now + 100, now, value)
        assert records(b) == ([(0, level - 1, level, HIGH_CONFIDENCE, before, value, F(0.95))] if i < 3 else [])
        before = value
    assert dynref.threshold(0.8, 0, 0.1).tobytes() == F(0.8).tobytes()
    assert [dynref.threshold(0.8, lv, 0.1) for lv in (1, 2, 3)] == [F(0.6), F(0.4), F(0.2)]


def test_min_clamp():
    b = bank([0.8], min_threshold=0.3, cooldown=0)
    assert [hit(b, t, 0.95).size and state(b)[4] for t in (0, 1, 2)] == [F(0.6), F(0.4), F(0.3)]
    assert records(b) == [(0, 2, 3, HIGH_CONFIDENCE, F(0.4), F(0.3), F(0.95))]
    # a min above the base raises the threshold of a learnt class above its base
    b = bank([0.5], trigger=0.6, min_threshold=0.7, cooldown=0)
    hit(b, 0, 0.65)
    assert state(b)[4] == F(0.7) and hit(b, 1, 0.69).size == 0 and hit(b, 2, 0.71).size == 1


def test_trigger_and_base_equalities():
    """x == trigger does not learn (strict); x == base learns (>=), which needs a lowered threshold for the hit to be one at all;
    trigger < x < base is approved by the lowered threshold and neither learns nor touches."""
    b = bank([0.8], trigger=0.9)
    assert hit(b, 0, 0.9).size == 1 and state(b) == (0, 0, 0, -1, F(0.8)) and records(b) == []
    b = bank([0.95], trigger=0.9, cooldown=0)
    assert hit(b, 0, 0.95).size == 0                                        # not above its own base: no event
    assert hit(b, 1, 0.96).size == 1 and state(b)[:4] == (1, 1, 101, 1)
    assert hit(b, 5, 0.92).size == 1 and state(b)[:4] == (1, 1, 101, 1)     # approved under 0.7125; below the base: nothing moves
    assert hit(b, 7, 0.95).size == 1 and state(b)[:4] == (2, 2, 107, 7)     # x == base learns


def test_cooldown_edges():
    b = bank([0.8], cooldown=10)
    hit(b, 5, 0.95)
    assert hit(b, 14, 0.95).size == 1 and state(b)[:4] == (1, 1, 114, 5) and records(b) == []     # cooldown - 1: kept alive, not learnt
    assert hit(b, 15, 0.95).size == 1 and state(b)[:4] == (2, 2, 115, 15)                         # cooldown: learnt


def test_expiry_edges():
    b = bank([0.8, 0.8], valid=100)
    hit(b, 0, 0.95)
    hit(b, 0, 0.95, c=1)
    assert state(b)[:3] == (1, 1, 100)
    assert hit(b, 100, 0.7).size == 1 and state(b)[:4] == (1, 1, 100, 0)    # now == E: still lowered; below the base: not touched
    assert hit(b, 101, 0.7).size == 0                                       # E + 1: reset before the hit is judged
    assert state(b) == (0, 0, 100, -1, F(0.8)) and state(b, 1)[0] == 0
    assert records(b) == [(0, 1, 0, EXPIRY, F(0.6), F(0.8), F(0)), (1, 1, 0, EXPIRY, F(0.6), F(0.8), F(0))]
    # a touch above the base keeps it alive; expiry and a new learning in one call are two records, the expiry first
    b = bank([0.8], valid=100, cooldown=0)
    hit(b, 0, 0.95)
    assert hit(b, 50, 0.85).size == 1 and state(b)[:4] == (1, 1, 150, 0)
    assert hit(b, 151, 0.95).size == 1 and state(b)[:4] == (1, 1, 251, 151)
    assert records(b) == [(0, 1, 0, EXPIRY, F(0.6), F(0.8), F(0)), (0, 0, 1, HIGH_CONFIDENCE, F(0.8), F(0.6), F(0.95))]


def test_a_class_that_is_not_dynamic():
    b = bank([0.8, 0.8], class_dynamic=[1, 0], cooldown=0)
    for t in range(3):
        assert hit(b, t, 0.99, c=1).size == 1
    assert state(b, 1) == (0, 0, 0, -1, F(0.8)) and records(b) == []
    b.restore_thresholds([0, 2], [0, 2], [0, 5], [-1, 1])                   # its state is kept and ignored
    assert hit(b, 50, 0.7, c=1).size == 0 and state(b, 1) == (2, 2, 5, 1, F(0.8))
    with pytest.raises(ValueError):
        b.restore_thresholds([0, 2], [0, 3], [0, 5], [-1, 1])
    b.reset_thresholds(1)
    assert state(b, 1) == (0, 0, 0, -1, F(0.8))
    with pytest.raises(ValueError):
        b.set_now(49)


def test_nan_and_inf_bases_stay_shut():
    b = bank([np.nan, np.inf], trigger=0.5, cooldown=0)
    for c in (0, 1):
        assert hit(b, c, 0.99, c=c).size == 0
    cur = b.thresholds()[4]
    assert np.isnan(cur[0]) and cur[1] == np.inf and records(b) == []
    assert np.isnan(dynref.threshold(np.nan, 2, 0.1)) and dynref.threshold(np.inf, 3, 0.1) == np.inf


@pytest.mark.parametrize("hold", [1, 3])
def test_no_dynamic_class_is_the_plain_rule(hold):
    rng = np.random.default_rng(hold)
    n_src, n_win, n_classes, k = 3, 30, 12, 4
    conf, idx = topk_rows(rng, n_src, n_win, n_classes, k)
    flt = filters(rng, n_classes, hold, 2, True, 1)
    plain = evbankref.EventBank(n_src, n_classes, k, flt)
    for dyn in (host.EventDynamic(np.zeros(n_classes, np.uint8), 0.1, 0.05, 5, 0), None):
        d = dynref.DynamicBank(evbankref.EventBank(n_src, n_classes, k, flt), dyn)
        plain.reset()
        a = feed(plain, conf, idx, "groups", np.random.default_rng(7))
        b = feed(d, conf, idx, "groups", np.random.default_rng(7))
        assert len(a) == len(b) and all(np.array_equal(x[0], y[0]) for x, y in zip(a, b))
        assert np.array_equal(plain.flush(), d.flush()) and d.take_changes().size == 0 and not d.thresholds()[0].any()


def test_two_sources_one_learning():
    """Two sources approve one class in one call: one learning, confidence the larger, whatever order the rows come in."""
    got = []
    for order in ([0, 1], [1, 0]):
        b = bank([0.8], cooldown=0)
        b.set_now(3)
        x = {0: 0.91, 1: 0.97}
        ev = b.process(order, np.array([[x[s]] for s in order], np.float32), np.zeros((2, 1), np.int32))
        assert ev.size == 2
        got.append((state(b), records(b)))
    assert got[0] == got[1] and got[0] == ((1, 1, 103, 3, F(0.6)), [(0, 0, 1, HIGH_CONFIDENCE, F(0.8), F(0.6), F(0.97))])


def test_a_refused_call_changes_no_class():
    b = bank([0.8], cooldown=0)
    hit(b, 0, 0.95)
    before, rec = state(b), records(b)
    b.set_now(500)
    with pytest.raises(evbankref.TooSmall):
        b.process([0], np.array([[0.95]], np.float32), np.zeros((1, 1), np.int32), cap=0)
    assert state(b) == before and records(b) == rec
    assert b.process([0], np.array([[0.95]], np.float32), np.zeros((1, 1), np.int32), cap=1).size == 1
    assert state(b)[:4] == (1, 1, 600, 500) and len(records(b)) == 2
    b.pending()
    assert len(records(b)) == 2
