"""File analysis of recordings at their own rates and depths, the part that needs no device: bnhip_analyze_mixed_windows is
bnhip_resample_length per recording followed by bnhip_analyze_windows, and the three entries answer argument errors before any
device is touched.  The burst of tests/test_analyze_mixed.py is stated here (BURST), with the facts about its lengths that make it
a test of the resample kernel's tiling."""
import ctypes as C

import numpy as np
import pytest

from birdnet_go_amd import host

MODEL_RATE, CLIP, HOP, MIN_TAIL, K = 48000, 12000, 6000, 7000, 5
TILE = 4096                                               # RESAMPLE_SLOT_TILE (csrc/resample.h): outputs of one block
# (rate, bits, samples at that rate): 160/147 upsampling, 1/2 (one phase, 41 taps), 3/2, the convert-only branch, 24/125 (105 taps
# per phase, the longest span), a recording shorter than the filter, and a long one that brings W above 64
BURST = [(44100, 16, 7526), (96000, 24, 8193), (32000, 32, 16002), (48000, 16, 31001), (250000, 0, 70000), (44100, 16, 7),
         (44100, 16, 300000)]
N_OUT = [8192, 4097, 24003, 31001, 13440, 8, 326531]
FIRST = [0, 1, 2, 5, 10, 12, 13, 67]


def burst_recs(burst=BURST):
    return host.recordings([n for _, _, n in burst], [r for r, _, _ in burst], [b for _, b, _ in burst])


def test_burst_facts(built_lib):
    """(CPU) the lengths at the model's rate and what they are there for, next to the table of the entry itself."""
    first, n_out = host.analyze_mixed_windows(burst_recs(), MODEL_RATE, CLIP, HOP, MIN_TAIL)
    assert n_out.tolist() == N_OUT and first.tolist() == FIRST
    assert N_OUT[0] == 2 * TILE and N_OUT[1] == TILE + 1 and N_OUT[2] % 4 == 3 and N_OUT[5] == 8
    # 24 003 = 3 hops + 6 003: the tail is below min_tail and dropped; 31 001 = 4 hops + 7 001: kept
    assert N_OUT[2] - 3 * HOP < MIN_TAIL and FIRST[3] - FIRST[2] == 3
    assert N_OUT[3] - 4 * HOP >= MIN_TAIL and FIRST[4] - FIRST[3] == 5
    W = FIRST[-1]
    assert W > 64 and W % 32 <= 16                        # three chunks at max_batch 32, the last one a small call
    assert FIRST[6] < 32                                  # the first chunk straddles all seven recordings


def _table_by_parts(recs, clip, hop, min_tail):
    lib = host.load_library()
    n_out = []
    for q in recs:
        n, rate = int(q["length"]), int(q["rate"])
        want = -(-n * (MODEL_RATE // np.gcd(rate, MODEL_RATE)) // (rate // np.gcd(rate, MODEL_RATE)))       # ceil(n * L / M), exact
        assert lib.bnhip_resample_length(n, rate, MODEL_RATE) == want
        n_out.append(int(want))
    return host.analyze_windows(n_out, clip, hop, min_tail), n_out


@pytest.mark.parametrize("hop,min_tail", [(HOP, MIN_TAIL), (HOP + 1, 0), (CLIP, CLIP)])
def test_mixed_windows_is_resample_length_then_windows(built_lib, hop, min_tail):
    recs = burst_recs()
    want_first, want_out = _table_by_parts(recs, CLIP, hop, min_tail)
    first, n_out = host.analyze_mixed_windows(recs, MODEL_RATE, CLIP, hop, min_tail)
    assert first.dtype == np.int64 and np.array_equal(first, want_first) and n_out.tolist() == want_out
    # resampled_length may be NULL
    lib = host._analyze_mixed_protos(host.load_library())
    out = np.zeros(len(recs) + 1, np.int64)
    assert lib.bnhip_analyze_mixed_windows(recs.ctypes.data, len(recs), MODEL_RATE, CLIP, hop, min_tail, out.ctypes.data, None) == first[-1]
    assert np.array_equal(out, first)


def test_mixed_windows_around_2_31(built_lib):
    """Lengths next to the 2^31 limit, in and out: 64-bit arithmetic, and the first refused value on either side."""
    big = (1 << 31) - 1
    recs = host.recordings([big, big, big - 1, (1 << 30), 1470001], [48000, 96000, 192000, 32000, 44100], 16)
    want_first, want_out = _table_by_parts(recs, 144000, 48000, 48000)
    first, n_out = host.analyze_mixed_windows(recs, MODEL_RATE, 144000, 48000, 48000)
    assert n_out.tolist() == want_out == [big, 1 << 30, (big - 1 + 3) // 4, 3 << 29, 1600002] and np.array_equal(first, want_first)
    edge = host.recordings([1431655764], [32000], [16])                   # * 3 / 2 = 2^31 - 2; one sample more gives ceil(2^31 - 0.5)
    assert host.analyze_mixed_windows(edge, MODEL_RATE, 144000, 48000, 48000)[1].tolist() == [big - 1]
    for length, rate in [(1 << 31, 48000), (1 << 31, 96000), (1431655765, 32000), (big, 44100)]:
        with pytest.raises(host.HipError) as ei:
            host.analyze_mixed_windows(host.recordings([length], [rate], [16]), MODEL_RATE, 144000, 48000, 48000)
        assert ei.value.code == host.E_INVALID and "2^31" in str(ei.value), (length, rate)


def _bad_tables():
    """(what is wrong, RECORDING table, model_rate): every refusal of the recordings themselves."""
    big = (1 << 31) - 1
    ok = [(44100, 16, 7526), (48000, 24, 100)]
    t = lambda rows: burst_recs(rows)
    return [("rate 0", t(ok + [(0, 16, 10)]), MODEL_RATE), ("rate < 0", t([(-44100, 16, 10)] + ok), MODEL_RATE),
            ("model_rate 0", t(ok), 0), ("model_rate < 0", t(ok), -48000),
            ("depth 8", t(ok + [(48000, 8, 10)]), MODEL_RATE), ("depth -16", t([(48000, -16, 10)]), MODEL_RATE),
            ("depth 64", t(ok + [(44100, 64, 10)]), MODEL_RATE),
            ("no samples", t(ok + [(48000, 16, 0)]), MODEL_RATE), ("negative length", t([(48000, 16, -5)]), MODEL_RATE),
            ("length 2^31", t(ok + [(48000, 16, 1 << 31)]), MODEL_RATE), ("n_out 2^31", t(ok + [(24000, 16, 1 << 30)]), MODEL_RATE),
            ("input total 2^36", t([(48000, 16, big)] * 33), MODEL_RATE),
            ("output total 2^36", t([(24000, 16, (1 << 30) - 1)] * 33), MODEL_RATE)]


def test_windows_argument_errors(built_lib):
    lib = host._analyze_mixed_protos(host.load_library())
    f = lib.bnhip_analyze_mixed_windows
    recs = burst_recs()
    first, n_out = np.full(len(recs) + 1, -7, np.int64), np.full(len(recs), -7, np.int64)
    P = lambda a: a.ctypes.data
    assert f(P(recs), len(recs), MODEL_RATE, CLIP, HOP, MIN_TAIL, P(first), P(n_out)) == FIRST[-1] and first.tolist() == FIRST
    first[:] = -7
    n_out[:] = -7
    for args in [(None, 7, MODEL_RATE, CLIP, HOP, 0), (P(recs), 0, MODEL_RATE, CLIP, HOP, 0), (P(recs), 65536, MODEL_RATE, CLIP, HOP, 0),
                 (P(recs), 7, MODEL_RATE, 0, 1, 0), (P(recs), 7, MODEL_RATE, CLIP, 0, 0), (P(recs), 7, MODEL_RATE, CLIP, CLIP + 1, 0),
                 (P(recs), 7, MODEL_RATE, CLIP, HOP, -1)]:
        assert f(*args, P(first), P(n_out)) == host.E_INVALID, args
    assert f(P(recs), 7, MODEL_RATE, CLIP, HOP, 0, None, P(n_out)) == host.E_INVALID
    for what, bad, model_rate in _bad_tables():
        assert f(P(bad), len(bad), model_rate, CLIP, HOP, 0, P(first), P(n_out)) == host.E_INVALID, what
    assert (first == -7).all() and (n_out == -7).all()    # nothing written by a refused call
    # fewer than 2^36 samples on both sides is no refusal: 32 recordings one sample short of 2^31
    many = host.recordings([(1 << 31) - 1] * 32, 48000, 16)
    assert host.analyze_mixed_windows(many, MODEL_RATE, 144000, 144000)[0][-1] == 32 * 14914


def test_entries_refuse_on_a_plan_only_handle(built_lib, tiny_blob):
    """bnhip_analyze_mixed_pcm_topk / bnhip_analyze_mixed_pcm: a well-formed call on a handle without a device is BNHIP_E_INVALID
    ("plan-only", the sentinel of the existing entries); every argument error is answered for the argument, with nothing written;
    the handle answers describe() afterwards."""
    lib = host._analyze_mixed_protos(host.load_library())
    m = host.HipClassifier(tiny_blob, plan_only=True)
    try:
        n = m.n_samples
        recs = host.recordings([2 * n, n + 5], [44100, 48000], [16, 24])
        pcm = np.zeros(2 * n * 2 + (n + 5) * 3, np.uint8)
        conf, idx = np.full((8, 5), -7, np.float32), np.full((8, 5), -7, np.int32)
        rows = np.zeros(40, host.DETECTION)
        rows["window"] = -7
        n_out = C.c_size_t(12345)
        P = lambda a: a.ctypes.data
        topk = lambda h=m._h, x=P(pcm), rc=recs, nr=None, rate=MODEL_RATE, hop=n // 2, mt=0, act=0, k=5, oc=P(conf), oi=P(idx): \
            lib.bnhip_analyze_mixed_pcm_topk(h, x, None if rc is None else P(rc), len(rc) if nr is None else nr, rate, hop, mt, act, 1.0, k, oc, oi)
        det = lambda h=m._h, x=P(pcm), rc=recs, nr=None, rate=MODEL_RATE, hop=n // 2, mt=0, act=0, k=5, o=P(rows), cap=40, no=C.byref(n_out): \
            lib.bnhip_analyze_mixed_pcm(h, x, None if rc is None else P(rc), len(rc) if nr is None else nr, rate, hop, mt, act, 1.0, k, 0.0, o, cap, no)
        for f in (topk, det):
            assert f() == host.E_INVALID                                   # well-formed, but the handle cannot run
            assert b"plan-only" in lib.bnhip_last_error()
            kws = [dict(h=None), dict(x=None), dict(rc=None, nr=2), dict(nr=0), dict(nr=65536), dict(hop=0), dict(hop=n + 1), dict(mt=-1),
                   dict(k=0), dict(act=3)]
            kws += [dict(rc=bad, rate=rate) for _, bad, rate in _bad_tables()]
            for kw in kws:
                assert f(**kw) == host.E_INVALID, kw
                assert b"plan-only" not in lib.bnhip_last_error(), kw       # (refused for the argument, not for the handle)
        assert topk(oc=None) == host.E_INVALID and topk(oi=None) == host.E_INVALID
        assert det(no=None) == host.E_INVALID and det(o=None) == host.E_INVALID
        assert (conf == -7).all() and (idx == -7).all() and (rows["window"] == -7).all() and n_out.value == 12345
        with pytest.raises(host.HipError):
            m.analyze_mixed_pcm_topk(pcm[:-1].tobytes(), recs, MODEL_RATE, n // 2)        # the bytes do not match the recordings
        with pytest.raises(host.HipError):
            m.analyze_mixed_pcm(pcm.tobytes(), host.recordings([2 * n, n + 5], [44100, 48000], [16, 8]), MODEL_RATE, n // 2)
        assert m.describe()["n_samples"] == n
    finally:
        m.close()
    multi = host.HipClassifier(tiny_blob, plan_only=True, devices=[0, 0])
    try:
        assert lib.bnhip_analyze_mixed_pcm_topk(multi._h, P(pcm), P(recs), 2, MODEL_RATE, n // 2, 0, 0, 1.0, 5, P(conf), P(idx)) == host.E_INVALID
        assert b"single-device" in lib.bnhip_last_error()
    finally:
        multi.close()
