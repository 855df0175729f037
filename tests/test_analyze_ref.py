"""File analysis, the part that needs no device: bnhip_analyze_windows / wav.window_table state wav.frame_clips' framing rule in
integers (a window is kept when it is the recording's first, or a whole clip remains, or at least min_tail samples remain; framing
stops once no more than a clip remains), and the three entries answer argument errors before any device is touched."""
import ctypes as C

import numpy as np
import pytest

from birdnet_go_amd import host, wav

CLIP = 24
LENGTHS = lambda hop, mt: [1, CLIP - 1, CLIP, CLIP + 1, CLIP + mt - 1, CLIP + mt, 2 * CLIP + hop]
HOPS = [1, 3, CLIP // 2, CLIP]
TAILS = [0, 1, CLIP // 3]


def _starts(length, hop, min_tail):
    """Sample offsets of frame_clips' windows (rate 1: seconds are samples)."""
    return wav.frame_clips(np.zeros(length, np.float32), 1, CLIP, CLIP - hop, min_tail)[1].astype(np.int64)


@pytest.mark.parametrize("hop", HOPS)
@pytest.mark.parametrize("min_tail", TAILS)
def test_window_table_is_frame_clips(built_lib, hop, min_tail):
    """Every edge of the rule, each length alone and all of them in one table: the counts are frame_clips', and window j of a
    recording starts at j * hop."""
    lengths = [n for n in LENGTHS(hop, min_tail) if n >= 1]
    want = [_starts(n, hop, min_tail) for n in lengths]
    for n, st in zip(lengths, want):
        assert np.array_equal(st, np.arange(st.size) * hop), (n, st)
        one = host.analyze_windows([n], CLIP, hop, min_tail)
        assert one.tolist() == [0, st.size], (n, hop, min_tail, one)
    first = host.analyze_windows(lengths, CLIP, hop, min_tail)
    assert first.dtype == np.int64 and first.tolist() == [0] + np.cumsum([st.size for st in want]).tolist()
    got, clip_len, got_hop, got_tail = wav.window_table(lengths, 1, CLIP, CLIP - hop, min_tail)
    assert (clip_len, got_hop, got_tail) == (CLIP, hop, min_tail) and np.array_equal(got, first)


def test_window_table_at_file_scale(built_lib):
    """An hour at 48 kHz, overlap 2 s, beside the default-tail cases of analyze_file: closed form, no loop over windows."""
    first, clip_len, hop, min_tail = wav.window_table([172_800_000], 48000, 3.0, 2.0)
    assert (clip_len, hop, min_tail) == (144000, 48000, 48000)
    assert first.tolist() == [0, 3598]                    # starts 0 s .. 3597 s: the last one holds exactly a clip
    first = wav.window_table([144_000 + 47_999, 144_000 + 48_000], 48000, 3.0, 0.0)[0]
    assert first.tolist() == [0, 1, 3]                    # a tail one sample short of the default second is dropped


def _raw(lib, name):
    f = getattr(lib, name)
    f.restype = C.c_longlong if name == "bnhip_analyze_windows" else C.c_int
    return f


def test_windows_argument_errors(built_lib):
    lib = host._analyze_protos(host.load_library())
    f = _raw(lib, "bnhip_analyze_windows")
    ln = np.array([100, 7], np.int64)
    out = np.full(3, -7, np.int64)
    ok = lambda lengths, n, clip, hop, mt, o: f(lengths, n, clip, hop, mt, o)
    assert ok(ln.ctypes.data, 2, 24, 12, 0, out.ctypes.data) == 9 and out.tolist() == [0, 8, 9]
    out[:] = -7
    for args in [(None, 2, 24, 12, 0, out.ctypes.data), (ln.ctypes.data, 2, 24, 12, 0, None), (ln.ctypes.data, 0, 24, 12, 0, out.ctypes.data),
                 (ln.ctypes.data, 65536, 24, 12, 0, out.ctypes.data), (ln.ctypes.data, 2, 24, 0, 0, out.ctypes.data),
                 (ln.ctypes.data, 2, 24, 25, 0, out.ctypes.data), (ln.ctypes.data, 2, 24, 12, -1, out.ctypes.data),
                 (ln.ctypes.data, 2, 0, 1, 0, out.ctypes.data)]:
        assert ok(*args) == host.E_INVALID, args
    bad = np.array([100, 0], np.int64)
    assert ok(bad.ctypes.data, 2, 24, 12, 0, out.ctypes.data) == host.E_INVALID
    huge = np.array([1 << 35, 1 << 35], np.int64)
    assert ok(huge.ctypes.data, 2, 24, 12, 0, out.ctypes.data) == host.E_INVALID
    assert out.tolist() == [-7, -7, -7]                  # nothing written by a refused call
    with pytest.raises(host.HipError):
        host.analyze_windows([10], 24, 25)


def test_entries_refuse_on_a_plan_only_handle(built_lib, tiny_blob):
    """bnhip_analyze_pcm_topk / bnhip_analyze_pcm: every argument error, and the plan-only handle itself, is BNHIP_E_INVALID with
    nothing written; the handle answers describe() afterwards."""
    lib = host._analyze_protos(host.load_library())
    m = host.HipClassifier(tiny_blob, plan_only=True)
    try:
        n = m.n_samples
        pcm = np.zeros(2 * n, np.int16)
        ln = np.array([2 * n], np.int64)
        conf, idx = np.full((3, 5), -7, np.float32), np.full((3, 5), -7, np.int32)
        rows = np.zeros(15, host.DETECTION)
        rows["window"] = -7
        n_out = C.c_size_t(12345)
        P = lambda a: a.ctypes.data
        topk = lambda h=m._h, x=P(pcm), bits=16, lens=P(ln), nr=1, hop=n // 2, mt=0, act=0, k=5, oc=P(conf), oi=P(idx): \
            lib.bnhip_analyze_pcm_topk(h, x, bits, lens, nr, hop, mt, act, 1.0, k, oc, oi)
        det = lambda h=m._h, x=P(pcm), bits=16, lens=P(ln), nr=1, hop=n // 2, mt=0, act=0, k=5, o=P(rows), cap=15, no=C.byref(n_out): \
            lib.bnhip_analyze_pcm(h, x, bits, lens, nr, hop, mt, act, 1.0, k, 0.0, o, cap, no)
        for f in (topk, det):
            assert f() == host.E_INVALID                                   # well-formed, but the handle cannot run
            assert b"plan-only" in lib.bnhip_last_error()
            for kw in [dict(h=None), dict(x=None), dict(lens=None), dict(bits=8), dict(bits=-16), dict(nr=0), dict(nr=65536), dict(hop=0),
                       dict(hop=n + 1), dict(mt=-1), dict(k=0), dict(act=3)]:
                assert f(**kw) == host.E_INVALID, kw
                assert b"plan-only" not in lib.bnhip_last_error(), kw       # (refused for the argument, not for the handle)
        assert topk(oc=None) == host.E_INVALID and topk(oi=None) == host.E_INVALID
        assert det(no=None) == host.E_INVALID and det(o=None) == host.E_INVALID
        assert (conf == -7).all() and (idx == -7).all() and (rows["window"] == -7).all() and n_out.value == 12345
        with pytest.raises(host.HipError):
            m.analyze_pcm_topk(pcm.tobytes(), 16, [2 * n + 1], n // 2)      # the bytes do not match the lengths
        assert m.describe()["n_samples"] == n
    finally:
        m.close()
    multi = host.HipClassifier(tiny_blob, plan_only=True, devices=[0, 0])
    try:
        assert lib.bnhip_analyze_pcm_topk(multi._h, P(pcm), 16, P(ln), 1, n // 2, 0, 0, 1.0, 5, P(conf), P(idx)) == host.E_INVALID
        assert b"single-device" in lib.bnhip_last_error()
    finally:
        multi.close()
