"""The span rule of the detection-clip entries on the host (bnhip_event_clip_spans) against its restatement (tests/clipref.py), on
crafted events; the float32 -> int16 rule of the restatement on the values that decide it; and the three entries' symbols.  No device."""
import ctypes as C

import numpy as np
import pytest

from birdnet_go_amd import host, wav

import clipref

HOP = 6000


def _events(items):
    """[(recording, first_window, last_window, status), ...] -> EVENT (the other fields do not enter the rule)."""
    ev = np.zeros(len(items), host.EVENT)
    for i, (r, fw, lw, st) in enumerate(items):
        ev[i] = (r, 3, fw, lw, fw, lw - fw + 1, 0.75, st)
    return ev


def _both(ev, lengths, pre, post, most, extended, hop=HOP):
    got = host.event_clip_spans(ev, lengths, hop, host.ClipSettings(pre, post, most, extended))
    want = clipref.spans(ev, lengths, hop, pre, post, most, extended)
    assert got.dtype == host.CLIP_SPAN and np.array_equal(got, want), (got, want)
    return got


def test_symbols_exported():
    lib = host.load_library()
    for s in ("bnhip_event_clip_spans", "bnhip_recording_clips_pcm16", "bnhip_analyze_channels_pcm_clips"):
        assert s in host.SYMBOLS and getattr(lib, s)


def test_clamps_and_short_recordings():
    lengths = [100 * HOP + 17, 7, 3 * HOP]
    ev = _events([(0, 0, 0, 0),          # begin clamps at sample 0
                  (0, 1, 1, 0),          # begin inside: hop - pre
                  (0, 99, 99, 0),        # end clamps at N
                  (0, 100, 100, 0),      # the last window: 17 samples of recording behind its start
                  (1, 0, 0, 0),          # a 7-sample recording: both clamps
                  (2, 2, 2, 0)])
    got = _both(ev, lengths, pre=4000, post=9000, most=2 ** 31 - 1, extended=False)
    assert got["start"].tolist() == [0, 2000, 99 * HOP - 4000, 100 * HOP - 4000, 0, 2 * HOP - 4000]
    assert got["length"].tolist() == [9000, 13000, 4000 + HOP + 17, 4000 + 17, 7, 4000 + HOP]
    assert (got["length"] >= 1).all() and got["recording"].tolist() == [0, 0, 0, 0, 1, 2]


def test_extended_end_and_the_cut():
    lengths = [100 * HOP]
    ev = _events([(0, 10, 10, 0), (0, 10, 14, 0), (0, 10, 90, 0)])
    normal = _both(ev, lengths, pre=3000, post=12000, most=2 ** 31 - 1, extended=False)
    assert normal["length"].tolist() == [15000] * 3                       # the end follows first_window
    ext = _both(ev, lengths, pre=3000, post=12000, most=2 ** 31 - 1, extended=True)
    assert ext["length"].tolist() == [15000, 15000 + 4 * HOP, 15000 + 80 * HOP]
    cut = _both(ev, lengths, pre=3000, post=12000, most=20000, extended=True)
    assert cut["length"].tolist() == [15000, 20000, 20000] and cut["start"].tolist() == [10 * HOP - 3000] * 3
    one = _both(ev, lengths, pre=0, post=1, most=1, extended=False)
    assert one["length"].tolist() == [1, 1, 1] and one["start"].tolist() == [10 * HOP] * 3


def test_dropped_events_have_no_clip():
    ev = _events([(0, 1, 1, 0), (0, 2, 2, 1), (0, 3, 3, 2), (0, 4, 4, 0)])
    got = _both(ev, [50 * HOP], pre=100, post=200, most=1000, extended=False)
    assert got["length"].tolist() == [300, 0, 0, 300]


def test_sweep():
    rng = np.random.default_rng(3)
    lengths = [7, 5 * HOP + 3, 40 * HOP + 1, HOP]
    items = []
    for _ in range(300):
        r = int(rng.integers(0, 4))
        last = max((lengths[r] - 1) // HOP, 0)
        fw = int(rng.integers(0, last + 1))
        items.append((r, fw, int(rng.integers(fw, last + 1)), int(rng.integers(0, 3))))
    ev = _events(items)
    for pre, post, most, ext in [(0, 1, 1, 0), (3 * HOP, 12 * HOP, 2 ** 31 - 1, 0), (HOP // 2, HOP + 1, 4 * HOP, 1), (7, 9, 13, 1)]:
        got = _both(ev, lengths, pre, post, most, bool(ext))
        kept = ev["status"] == 0
        assert (got["length"][kept] >= 1).all() and (got["length"][~kept] == 0).all()
        assert (got["start"] + got["length"] <= np.asarray(lengths)[got["recording"]]).all()


def test_refusals_write_nothing():
    lib = host._analyze_clips_protos(host.load_library())
    ev = _events([(0, 1, 1, 0), (1, 0, 0, 0)])
    lengths = np.array([50 * HOP, 7], np.int64)
    good = host.ClipSettings(100, 200, 1000)

    def call(events=ev, n=None, ln=lengths, n_rec=2, hop=HOP, x=good, with_spans=True):
        spans = np.full(ev.size, -7, host.CLIP_SPAN)
        xs = x._struct() if x is not None else None
        rc = lib.bnhip_event_clip_spans(events.ctypes.data if events is not None else None, ev.size if n is None else n,
                                        ln.ctypes.data if ln is not None else None, n_rec, hop, C.addressof(xs) if xs is not None else None,
                                        spans.ctypes.data if with_spans else None)
        return rc, spans

    rc, spans = call()
    assert rc == host.BNHIP_OK and (spans["length"] == 300).any()
    untouched = np.full(ev.size, -7, host.CLIP_SPAN)
    bad = [dict(events=None), dict(ln=None), dict(x=None), dict(with_spans=False),
           dict(x=host.ClipSettings(-1, 200, 1000)), dict(x=host.ClipSettings(100, 0, 1000)), dict(x=host.ClipSettings(100, 200, 0)),
           dict(n_rec=1),                                                  # the second event's recording lies outside the table
           dict(events=_events([(0, 1, 1, 0), (-1, 0, 0, 0)]))]
    for kw in bad:
        rc, spans = call(**kw)
        assert rc == host.E_INVALID and np.array_equal(spans, untouched), kw
        assert lib.bnhip_last_error()


def test_float_to_int16_rule():
    """The restatement on the values that decide it: a 16-bit sample is itself, ties go to even, values beyond +-1 clamp, NaN is 0."""
    all16 = np.arange(-32768, 32768).astype(np.int16)
    assert np.array_equal(clipref.to_pcm16(all16.astype(np.float32) / np.float32(32768.0)), all16)
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 32766.5, 32767.5, -32768.5, 40000.0, -40000.0, np.inf, -np.inf, np.nan], np.float32) / np.float32(32768.0)
    assert clipref.to_pcm16(x).tolist() == [0, 2, 2, 0, -2, 32766, 32767, -32768, 32767, -32768, 32767, -32768, 0]
    # 24-bit words: the low byte rounds to nearest, ties to even
    w = np.array([0x000080, 0x000180, 0x000081, 0x7FFFFF, -0x800000, -0x000080, -0x000180], np.int64)
    raw = w.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    assert clipref.to_pcm16(clipref.as_float32(raw, 24)).tolist() == [0, 2, 1, 32767, -32768, 0, -2]


def test_wav_clip_spans_in_seconds():
    ev = _events([(0, 2, 5, 0)])
    x = wav.ClipExport(length_seconds=0.5, pre_capture_seconds=0.1)
    got = wav.clip_spans(ev, [100000], HOP, x, model_rate=48000)
    assert got.tolist() == [(2 * HOP - 4800, 24000, 0)]
    with pytest.raises(ValueError):
        wav.ClipExport(extended=True)
