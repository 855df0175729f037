"""The capture bank's rules on the host: the restatement (tests/capref.py) against CaptureBuffer.Write / ReadSegment of the reference
restated in sample positions (capref.GoCapture); the span rule on a running clock (bnhip_capture_spans) against the restatement and
against bnhip_event_clip_spans; its refusals; the new symbols.  No device."""
import ctypes as C

import numpy as np
import pytest

from birdnet_go_amd import host

import capref

HOP = 6000
STATUSES = (capref.OK, capref.CLAMPED, capref.NOT_YET, capref.GONE, capref.DROPPED)


def test_symbols_exported():
    lib = host.load_library()
    for s in ("bnhip_capture_bank_create", "bnhip_capture_bank_info", "bnhip_capture_bank_positions", "bnhip_capture_bank_reset",
              "bnhip_capture_bank_write", "bnhip_capture_bank_read_pcm16", "bnhip_capture_bank_clips", "bnhip_capture_bank_destroy",
              "bnhip_capture_spans"):
        assert s in host.SYMBOLS and getattr(lib, s)
    assert (host.CAPTURE_OK, host.CAPTURE_CLAMPED, host.CAPTURE_NOT_YET, host.CAPTURE_GONE, host.CAPTURE_DROPPED) == STATUSES


# ------------------------------------------------------------------------------------------ the ring against the reference's
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_ring_against_capture_go(seed):
    """The same writes into capref.Ring and capref.GoCapture.  Every segment the reference answers equals the restatement's read, its
    "insufficient data" is NOT_YET and its "empty after clamping" is GONE.

    The one stated difference: a write longer than the ring counts in full here (the clock stays audio time) and by its stored tail
    only in the reference (capture.go:148-152, 162) - so the reference's positions lag ours by the samples it did not count (`lag`),
    and the test asks it for the same audio at its own positions."""
    cap = 2048
    rng = np.random.default_rng(seed)
    ring, go = capref.Ring(cap), capref.GoCapture(cap)
    lag = n_long = answered = 0
    seen = set()
    sizes = [0, 1, cap, cap + 1, 5000, 7, cap - 1] + [int(n) for n in rng.integers(0, 900, 40)] + [3 * cap + 5] + [int(n) for n in rng.integers(0, 900, 20)]
    for n in sizes:
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        ring.write(x)
        go.write(x)
        if n > cap:
            lag += n - cap
            n_long += 1
        assert ring.written == go.total + lag                              # the difference, and nothing else
        for _ in range(12):
            start = int(rng.integers(ring.oldest() - 300, ring.written + 50))
            end = start + int(rng.integers(1, cap))                       # (below the whole ring: extractSegment answers an empty
            begin = max(start, ring.oldest())                             #  slice for start index == end index, capture.go:313-316)
            kind = capref.NOT_YET if end > ring.written else capref.GONE if begin >= end else capref.OK if begin == start else capref.CLAMPED
            seen.add(kind)
            try:
                got = go.read_segment(start - lag, end - lag)
            except capref.GoError as e:
                assert (e.kind, kind) in (("insufficient", capref.NOT_YET), ("empty after clamping", capref.GONE)) or \
                    (e.kind == "no data" and ring.written == 0), (e.kind, kind, start, end)
                continue
            assert kind in (capref.OK, capref.CLAMPED) and np.array_equal(got, ring.read(begin, end - begin)), (start, end)
            answered += 1
    assert n_long >= 3 and answered > 100 and seen == {capref.OK, capref.CLAMPED, capref.NOT_YET, capref.GONE}


def test_write_trim_and_oldest():
    r = capref.Ring(1024)
    r.write(np.arange(1000, dtype=np.int16))
    assert (r.written, r.oldest()) == (1000, 0)
    r.write(np.arange(1000, 4000, dtype=np.int16))                       # longer than the ring: every sample counts, the last 1024 stay
    assert (r.written, r.oldest()) == (4000, 2976)
    assert np.array_equal(r.read(2976, 1024), np.arange(2976, 4000, dtype=np.int16))
    r.floor = 3500                                                        # (what a failed write leaves)
    assert r.oldest() == 3500
    r.reset()
    assert (r.written, r.oldest()) == (0, 0)
    assert capref.capacity(1) == 1024 and capref.capacity(1024) == 1024 and capref.capacity(1025) == 2048


def test_pcm16_rule():
    """16 bits: the identity.  24 and 32 bits: ties to even, and saturation at +32767 (the largest inputs round up to 2^15)."""
    x = np.array([-32768, -1, 0, 1, 32767], "<i2")
    assert np.array_equal(capref.pcm16(x.tobytes(), 16), x)
    v24 = np.array([0x80, 0x180, 0x280, -0x80, -0x180, 0x7FFFFF, -0x800000, 0x7FFF7F, 0x7FFF80], np.int32)   # x.5 ties; the ends
    b24 = np.stack([(v24 >> s) & 0xFF for s in (0, 8, 16)], 1).astype(np.uint8).tobytes()
    assert capref.pcm16(b24, 24).tolist() == [0, 2, 2, 0, -2, 32767, -32768, 32767, 32767]
    v32 = np.array([0x8000, 0x18000, -0x8000, -0x18000, 0x7FFFFFFF, -0x80000000, 0x7FFF8000], np.int64).astype("<i4")
    assert capref.pcm16(v32.tobytes(), 32).tolist() == [0, 2, 0, -2, 32767, -32768, 32767]


# ------------------------------------------------------------------------------------------ the span rule
def _events(rng, n, n_sources, max_window):
    ev = np.zeros(n, host.EVENT)
    ev["recording"] = rng.integers(0, n_sources, n)
    ev["class_index"] = rng.integers(0, 50, n)
    ev["first_window"] = rng.integers(0, max_window, n)
    ev["last_window"] = ev["first_window"] + rng.integers(0, 6, n)
    ev["best_window"], ev["count"], ev["confidence"] = ev["first_window"], 1, 0.5
    ev["status"] = rng.choice([0, 0, 0, 0, 1, 2], n)
    return ev


@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("most", [2 ** 31 - 1, 20000], ids=["uncut", "cut"])
def test_capture_spans_random(extended, most):
    rng = np.random.default_rng(5 + extended + most % 7)
    n_sources, cap = 5, 40 * HOP
    written = np.array([0, 30 * HOP, 100 * HOP + 17, 250 * HOP, 90 * HOP], np.int64)
    oldest = np.maximum(0, written - cap)
    oldest[4] = 70 * HOP + 3                                              # a raised floor
    ev = _events(rng, 2000, n_sources, 260)
    settings = host.ClipSettings(9000, 12000, most, extended)
    seen, cut = set(), 0
    for origins in (None, np.zeros(n_sources, np.int64), np.array([-3000, 3000, -HOP // 2, 12345, -1], np.int64)):
        got, status = host.capture_spans(ev, written, oldest, HOP, settings, origins)
        want, wstatus = capref.spans(ev, written, oldest, HOP, 9000, 12000, most, extended, origins)
        assert got.dtype == host.CLIP_SPAN and np.array_equal(got, want) and np.array_equal(status, wstatus)
        has = np.isin(status, (capref.OK, capref.CLAMPED))
        assert (got["length"][has] >= 1).all() and (got["length"][~has] == 0).all()
        assert (got["start"][has] >= oldest[got["recording"][has]]).all()
        assert (got["start"][has] + got["length"][has] <= written[got["recording"][has]]).all()
        seen |= set(status.tolist())
        cut += int((got["length"][has] == most).sum())
    assert seen == set(STATUSES)
    assert (cut > 0) == (most == 20000)                                   # max_samples binds in the cut cases (pre + post = 21000) only


def test_capture_spans_is_the_file_rule_on_a_full_clock():
    """written = N, oldest = 0, origins = 0: wherever the end lies inside the recording, the span is bnhip_event_clip_spans's."""
    rng = np.random.default_rng(11)
    lengths = np.array([100 * HOP + 17, 7, 3 * HOP, 260 * HOP], np.int64)
    ev = _events(rng, 2000, 4, 260)
    n_same = 0
    for extended in (False, True):
        for most in (2 ** 31 - 1, 15000):
            settings = host.ClipSettings(4000, 9000, most, extended)
            got, status = host.capture_spans(ev, lengths, np.zeros(4, np.int64), HOP, settings)
            filed = host.event_clip_spans(ev, lengths, HOP, settings)
            p1 = np.where(extended, ev["last_window"], ev["first_window"]).astype(np.int64) * HOP + 9000
            inside = p1 <= lengths[ev["recording"]]
            live = ev["status"] == 0
            assert np.array_equal(got[inside & live], filed[inside & live])
            assert np.isin(status[inside & live], (capref.OK, capref.CLAMPED)).all()
            assert (status[~inside & live] == capref.NOT_YET).all() and (status[~live] == capref.DROPPED).all()
            assert (filed["length"][~live] == 0).all() and (got["length"][~live] == 0).all()
            n_same += int((inside & live).sum())
    assert n_same > 1000


def test_capture_spans_refusals():
    lib = host._capture_bank_protos(host.load_library())
    ev = _events(np.random.default_rng(0), 4, 2, 10)
    wr, old = np.full(2, 10 ** 6, np.int64), np.zeros(2, np.int64)
    spans, status = np.zeros(4, host.CLIP_SPAN), np.zeros(4, np.int32)
    good = host.ClipSettings(100, 200, 1000)

    def call(events=ev, n=4, n_sources=2, written=wr, oldest=old, hop=HOP, settings=good, sp=spans, st=status):
        xs = settings._struct() if settings is not None else None
        P = lambda a: None if a is None else a.ctypes.data
        return lib.bnhip_capture_spans(P(events), n, n_sources, P(written), P(oldest), None, hop, None if xs is None else C.addressof(xs), P(sp), P(st))

    assert call() == host.BNHIP_OK
    assert call(events=None, n=0, sp=None, st=None) == host.BNHIP_OK      # no events: nothing to point at
    before = (spans.copy(), status.copy())
    for bad in (dict(events=None), dict(sp=None), dict(st=None), dict(written=None), dict(oldest=None), dict(settings=None),
                dict(n_sources=0), dict(hop=0), dict(settings=host.ClipSettings(-1, 200, 1000)), dict(settings=host.ClipSettings(100, 0, 1000)),
                dict(settings=host.ClipSettings(100, 200, 0))):
        assert call(**bad) == host.E_INVALID, bad
    outside = ev.copy()
    outside["recording"][2] = 2
    assert call(events=outside) == host.E_INVALID and b"source outside" in lib.bnhip_last_error()
    outside["recording"][2] = -1
    assert call(events=outside) == host.E_INVALID
    assert np.array_equal(spans, before[0]) and np.array_equal(status, before[1])       # a refusal writes nothing
    with pytest.raises(host.HipError):
        host.capture_spans(ev, wr, old[:1], HOP, good)
