"""File analysis of recordings at their own rates and depths in one device call (bnhip_analyze_mixed_pcm_topk / bnhip_analyze_mixed_pcm,
wav.analyze_files(device_resample=True)).

The criterion is bit identity - np.array_equal on conf and idx - with what wav.analyze_files builds on the host today: every
recording converted to float32 as wav.read_wav converts, resampled by bnhip_resample_f32 with n_clips = 1 (a copy at equal rates),
then ONE bnhip_analyze_pcm_topk(bits = 0) call over those float32 recordings on the same engine.  It is derived, not measured: a
resampled sample is resample_tile's fmaf chain over the same taps in the same order, dividing an integer's float32 by a power of
two is exact, int32 -> float32 rounds to nearest even in numpy and on the device alike, and both sides frame float32 slots of the
same layout in the same chunks.  No tolerance appears anywhere; the resampler's values stay pinned to scipy by tests/test_resample.py.

The burst (tests/test_analyze_mixed_ref.py BURST, whose length facts are asserted there and again here before any device work):
seven recordings of five rates and all four depths, 67 windows: chunks of 32, 32 and 3 at max_batch 32, the first straddling all
seven.  Which form a chunk took is read from the per-step profile as tests/test_analyze.py reads it: the float32 slots are read by
the framed min/max launch where they lie (4 + 4 bytes a sample)."""
import ctypes as C
import struct

import numpy as np
import pytest

from birdnet_go_amd import host, wav

from test_analyze import _fft_tiny_blob, _profiled, _minmax_bytes, _same
from test_analyze_mixed_ref import BURST, CLIP, FIRST, HOP, K, MIN_TAIL, MODEL_RATE, N_OUT, TILE, burst_recs

pytestmark = pytest.mark.gpu


def _wav_bytes(raw, rate, bits):
    return (b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, rate, rate * bits // 8, bits // 8, bits)
            + b"data" + struct.pack("<I", len(raw)) + raw)


def _material(burst, seed=23):
    """-> [(the recording's bytes as they are in a file, its float32 samples as wav.read_wav converts them)]: a tone and noise at a
    level of its own per recording, full-scale samples of both signs, and at 24 / 32 bits low bits that a 16-bit word does not have
    (the 32-bit words need rounding to become float32)."""
    rng = np.random.default_rng(seed)
    out = []
    for i, (rate, bits, n) in enumerate(burst):
        t = np.arange(n)
        x = (0.2 + 0.07 * i) * np.sin(2 * np.pi * (300.0 + 170.0 * i) * t / rate) + 0.05 * rng.standard_normal(n)
        x[:: max(n // 3, 1)] = -1.0
        x[1:: max(n // 2, 2)] = 1.0
        if bits == 0:
            s = x.astype(np.float32)
            out.append((s.tobytes(), s))
            continue
        full = 1 << (bits - 1)
        v = np.clip(np.round(x * (full - 1) * 0.9 + rng.integers(-3, 4, n)), -full, full - 1).astype(np.int64)
        v[x == -1.0], v[x == 1.0] = -full, full - 1
        raw = v.astype("<i2").tobytes() if bits == 16 else v.astype("<i4").tobytes() if bits == 32 else \
            v.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
        s, got_rate, got_bits = wav.read_wav(_wav_bytes(raw, rate, bits))
        assert (got_rate, got_bits, s.size) == (rate, bits, n)
        out.append((raw, s))
    return out


def _host_resampled(material, burst):
    """What wav.analyze_files builds for the burst today: every recording as float32 at the model's rate."""
    return [s if rate == MODEL_RATE else host.Resampler(rate, MODEL_RATE).resample_f32(s) for (_, s), (rate, _, _) in zip(material, burst)]


def _want(c, floats, hop=HOP, min_tail=MIN_TAIL, k=K):
    conf, idx, first = c.analyze_pcm_topk(np.concatenate(floats).astype(np.float32).tobytes(), 0, [x.size for x in floats], hop, min_tail, k=k)
    return conf, idx, first


@pytest.fixture(scope="module")
def burst(gpu):
    material = _material(BURST)
    floats = _host_resampled(material, BURST)
    assert [x.size for x in floats] == N_OUT
    return {"raw": b"".join(raw for raw, _ in material), "material": material, "floats": floats, "recs": burst_recs()}


@pytest.fixture(scope="module")
def engine(gpu, burst):
    c = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False, lanes=2)
    want = _want(c, burst["floats"])
    yield c, want
    c.close()


def test_mixed_burst(engine, burst):
    """Five rates, four depths, lanes 2 and 1.  Profiled (one lane), every chunk of 32 reads the float32 slots in the framed form."""
    first, n_out = host.analyze_mixed_windows(burst["recs"], MODEL_RATE, CLIP, HOP, MIN_TAIL)
    assert n_out.tolist() == N_OUT and first.tolist() == FIRST            # (CPU) the table, before any device work
    assert N_OUT[0] % TILE == 0 and N_OUT[1] == TILE + 1 and N_OUT[2] % 4 and N_OUT[5] == 8 < 21
    W = FIRST[-1]
    assert W > 64 and W % 32 <= 16 and FIRST[6] < 32                      # three chunks, the first straddling all the recordings
    c2, want2 = engine
    one = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False, lanes=1)
    try:
        for c, want in ((c2, want2), (one, _want(one, burst["floats"]))):
            got = c.analyze_mixed_pcm_topk(burst["raw"], burst["recs"], MODEL_RATE, HOP, MIN_TAIL, k=K)
            assert got[0].shape == (W, K) and np.array_equal(got[2], want[2]) and got[2].tolist() == FIRST
            _same(got[:2], want[:2])
            got, names = _profiled(c, lambda: c.analyze_mixed_pcm_topk(burst["raw"], burst["recs"], MODEL_RATE, HOP, MIN_TAIL, k=K))
            _same(got[:2], want[:2])
            assert _minmax_bytes(names) == (W - W % 32) * CLIP * (4 + 4) + (W % 32) * CLIP * 4, names["clip_minmax"]
    finally:
        one.close()
    # an odd hop: every chunk goes through k_frame_windows, which reads the slots sample by sample
    want = _want(c2, burst["floats"], HOP + 1)
    _same(c2.analyze_mixed_pcm_topk(burst["raw"], burst["recs"], MODEL_RATE, HOP + 1, MIN_TAIL, k=K)[:2], want[:2])


def test_permuted_order(engine, burst):
    """The recordings in another order (the raw block's slots and the float slots land elsewhere, a 24-bit recording now starts the
    block, the 7-sample one ends it): each recording's rows are what they were."""
    c, want = engine
    perm = [1, 6, 4, 0, 3, 2, 5]
    raw = b"".join(burst["material"][r][0] for r in perm)
    conf, idx, first = c.analyze_mixed_pcm_topk(raw, burst["recs"][perm], MODEL_RATE, HOP, MIN_TAIL, k=K)
    assert first[-1] == FIRST[-1]
    for j, r in enumerate(perm):
        a, b = slice(first[j], first[j + 1]), slice(FIRST[r], FIRST[r + 1])
        assert first[j + 1] - first[j] == FIRST[r + 1] - FIRST[r]
        _same((conf[a], idx[a]), (want[0][b], want[1][b]))


def test_fast_path_is_the_existing_call(engine, burst):
    """Every recording at the model's rate as int16: the rows of bnhip_analyze_pcm_topk(bits = 16), no float32 slots (the framed
    launch reads the int16 recordings: 2 + 4 bytes a sample) and no launch beyond that call's."""
    c, _ = engine
    rows = [(MODEL_RATE, 16, n) for n in N_OUT]
    material = _material(rows, seed=5)
    raw, lengths = b"".join(m[0] for m in material), [n for _, _, n in rows]
    want, names_want = _profiled(c, lambda: c.analyze_pcm_topk(raw, 16, lengths, HOP, MIN_TAIL, k=K))
    got, names = _profiled(c, lambda: c.analyze_mixed_pcm_topk(raw, burst_recs(rows), MODEL_RATE, HOP, MIN_TAIL, k=K))
    _same(got[:2], want[:2])
    W = FIRST[-1]
    assert np.array_equal(got[2], want[2]) and got[2][-1] == W
    assert _minmax_bytes(names) == (W - W % 32) * CLIP * (2 + 4) + (W % 32) * CLIP * 4, names["clip_minmax"]
    assert not [n for n in names if "resample" in n]
    assert {n: v["launches"] for n, v in names.items()} == {n: v["launches"] for n, v in names_want.items()}


def test_detection_rows(engine, burst):
    """bnhip_analyze_mixed_pcm's rows are bnhip_analyze_pcm's over the float32 recordings, field for field, for a threshold that
    keeps some rows and drops some; a cap below the total writes cap rows and reports the total; cap 0 takes out = NULL."""
    c, want = engine
    floats = burst["floats"]
    fraw, flen = np.concatenate(floats).tobytes(), [x.size for x in floats]
    mid = float(np.sort(want[0].reshape(-1))[want[0].size // 2])
    want_rows, want_total = c.analyze_pcm(fraw, 0, flen, HOP, MIN_TAIL, k=K, threshold=mid)
    assert 0 < want_total < want[0].size and want_rows.size == want_total
    assert len(set(want_rows["recording"].tolist())) > 1                   # rows of several recordings, windows counted inside each
    rows, total = c.analyze_mixed_pcm(burst["raw"], burst["recs"], MODEL_RATE, HOP, MIN_TAIL, k=K, threshold=mid)
    assert total == want_total and rows.tobytes() == want_rows.tobytes()
    rows, total = c.analyze_mixed_pcm(burst["raw"], burst["recs"], MODEL_RATE, HOP, MIN_TAIL, k=K, threshold=mid, cap=7)
    assert total == want_total > 7 and rows.tobytes() == want_rows[:7].tobytes()
    rows, total = c.analyze_mixed_pcm(burst["raw"], burst["recs"], MODEL_RATE, HOP, MIN_TAIL, k=K, threshold=mid, cap=0)
    assert total == want_total and rows.size == 0


def test_refusals_leave_the_handle_usable(engine, burst):
    """Every refusal of the recordings' table and of the call's arguments on a live handle: BNHIP_E_INVALID with nothing written;
    44 100 -> 256 000 Hz (L = 2 560 phases of 21 taps: 215 KB of table against 150 KB of LDS) is BNHIP_E_UNSUPPORTED and names the
    recording and both rates; a multi-device handle is refused; the handle then answers the burst as before.  (The refusal of more
    resample tiles than a 31-bit grid cannot be reached: 2^36 samples are at most 2^24 + 65 535 tiles of 4 096.)"""
    from test_analyze_mixed_ref import _bad_tables
    c, want = engine
    raw, recs = burst["raw"], burst["recs"]
    # (the C entries themselves: a refused table is answered before the samples are looked at, so a few bytes stand in for them)
    lib = host._analyze_mixed_protos(c._lib)
    some = np.zeros(64, np.uint8)
    conf, idx = np.full((8, K), -7, np.float32), np.full((8, K), -7, np.int32)
    det, n_det = np.zeros(8, host.DETECTION), C.c_size_t(12345)
    for what, bad, rate in _bad_tables():
        assert lib.bnhip_analyze_mixed_pcm_topk(c._h, some.ctypes.data, bad.ctypes.data, len(bad), rate, HOP, MIN_TAIL, 0, 1.0, K, conf.ctypes.data,
                                                idx.ctypes.data) == host.E_INVALID, what
        assert lib.bnhip_analyze_mixed_pcm(c._h, some.ctypes.data, bad.ctypes.data, len(bad), rate, HOP, MIN_TAIL, 0, 1.0, K, 0.0, det.ctypes.data, 8,
                                           C.byref(n_det)) == host.E_INVALID, what
    for null in ("h", "pcm", "recs", "out"):
        assert lib.bnhip_analyze_mixed_pcm_topk(None if null == "h" else c._h, None if null == "pcm" else some.ctypes.data,
                                                None if null == "recs" else recs.ctypes.data, len(recs), MODEL_RATE, HOP, MIN_TAIL, 0, 1.0, K,
                                                None if null == "out" else conf.ctypes.data, idx.ctypes.data) == host.E_INVALID, null
    for nr in (0, 65536):
        assert lib.bnhip_analyze_mixed_pcm_topk(c._h, some.ctypes.data, recs.ctypes.data, nr, MODEL_RATE, HOP, MIN_TAIL, 0, 1.0, K, conf.ctypes.data,
                                                idx.ctypes.data) == host.E_INVALID
    assert (conf == -7).all() and (idx == -7).all() and not det["confidence"].any() and n_det.value == 12345
    for kw in [dict(hop=0), dict(hop=CLIP + 1), dict(min_tail=-1), dict(k=0), dict(activation=3)]:
        args = dict(hop=HOP, min_tail=MIN_TAIL, k=K)
        args.update(kw)
        for call in (c.analyze_mixed_pcm_topk, c.analyze_mixed_pcm):
            with pytest.raises(host.HipError) as ei:
                call(raw, recs, MODEL_RATE, **args)
            assert ei.value.code == host.E_INVALID, kw
    # (CPU) the pair's LDS need, as resample_lds states it: (L * T + 255 * M / L + T + 2) floats
    L, M = 2560, 441
    T = (2 * 10 * L + 1 + L - 1) // L
    assert (L * T + 255 * M // L + T + 2) * 4 > 150 * 1024 and T == 21
    bat = host.recordings([7526, 1000, 500], [48000, 44100, 96000], [16, 16, 24])
    for call in (c.analyze_mixed_pcm_topk, c.analyze_mixed_pcm):
        with pytest.raises(host.HipError) as ei:
            call(np.zeros(7526 * 2 + 1000 * 2 + 500 * 3, np.uint8), bat, 256000, HOP, MIN_TAIL, k=K)
        assert ei.value.code == host.E_UNSUPPORTED and "recording 1" in str(ei.value) and "44100" in str(ei.value) and "256000" in str(ei.value)
    multi = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False, devices=[0, 0], replicate="peer")
    try:
        with pytest.raises(host.HipError) as ei:
            multi.analyze_mixed_pcm_topk(raw, recs, MODEL_RATE, HOP, MIN_TAIL, k=K)
        assert ei.value.code == host.E_INVALID and "single-device" in str(ei.value)
    finally:
        multi.close()
    _same(c.analyze_mixed_pcm_topk(raw, recs, MODEL_RATE, HOP, MIN_TAIL, k=K)[:2], want[:2])


def test_analyze_files_device_resample(gpu, tmp_path):
    """wav.analyze_files(device_resample=True) over WAV files of three rates and two depths: the rows of the default path, and
    analyze_file passes the keyword through.  (The table cache exposes nothing to assert a second call's reuse on; the second call
    is made, and must answer the same.)"""
    files = [(44100, 16, 30001), (96000, 24, 50003), (48000, 16, 2 * CLIP + 9000), (44100, 24, 13000)]
    paths = []
    for i, ((rate, bits, n), (raw, _)) in enumerate(zip(files, _material(files, seed=9))):
        paths.append(str(tmp_path / f"{i}.wav"))
        with open(paths[-1], "wb") as fh:
            fh.write(_wav_bytes(raw, rate, bits))
    c = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False)
    try:
        kw = dict(overlap_seconds=CLIP / 2 / MODEL_RATE, top_k=K, model_rate=MODEL_RATE)
        dense = wav.analyze_files(paths, c, **kw)
        thr = sorted(r[3] for rows in dense for r in rows)[sum(len(rows) for rows in dense) // 3]
        want = wav.analyze_files(paths, c, threshold=thr, **kw)
        assert 0 < sum(len(w) for w in want) < sum(len(d) for d in dense)
        got = wav.analyze_files(paths, c, threshold=thr, device_resample=True, **kw)
        assert got == want
        assert wav.analyze_files(paths, c, threshold=thr, device_resample=True, **kw) == want
        assert wav.analyze_file(paths[1], c, threshold=thr, device_framing=True, device_resample=True, **kw) == want[1]
        assert wav.analyze_file(paths[1], c, threshold=thr, **kw) == want[1]
    finally:
        c.close()


def test_full_model_real_offsets(gpu, full_blob):
    """The full model's 144 000-sample windows at hop 48 000 over a 44 100 Hz int16 and a 96 000 Hz 24-bit recording: 3 + 4 windows,
    each at an offset of its own into a resampled slot."""
    n, hop, mt = 144000, 48000, 48000
    rows = [(44100, 16, 200000), (96000, 24, 500001)]
    recs = burst_recs(rows)
    first, n_out = host.analyze_mixed_windows(recs, MODEL_RATE, n, hop, mt)
    assert n_out.tolist() == [217688, 250001] and first.tolist() == [0, 3, 7]      # (CPU)
    material = _material(rows, seed=4)
    floats = _host_resampled(material, rows)
    c = host.HipClassifier(full_blob, max_batch=32, autotune=False, lanes=1)
    try:
        assert c.n_samples == n
        want = _want(c, floats, hop, mt, 10)
        got = c.analyze_mixed_pcm_topk(b"".join(m[0] for m in material), recs, MODEL_RATE, hop, mt, k=10)
        assert np.array_equal(got[2], first)
        _same(got[:2], want[:2])
    finally:
        c.close()
