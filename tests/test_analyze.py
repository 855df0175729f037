"""File analysis with the windows framed on the device (bnhip_analyze_pcm_topk / bnhip_analyze_pcm, wav.analyze_file(device_framing=True)).

The criterion is bit identity - np.array_equal on conf and idx - with bnhip_predict_pcm_topk of the host-framed windows on the same
engine.  It is derived, not measured: a clip's outputs do not depend on how a call is cut (engine.h, the two-phase host calls),
min / max are exact whatever the grouping, k_clip_norm_resident is pinned to the min/max + normalise pair bit for bit
(tests/test_norm_resident.py), and a window's zero tail is the zeros wav.frame_clips pads with.

Which form a chunk took is read from the per-step profile, as tests/test_norm_resident.py reads it: the clip_minmax step's bytes are
bytes-per-sample + 4 per sample where the resident launch read the recording itself (the framed form), 4 + 4 where it read float
windows that k_frame_windows had written, and 4 where a lane of 16 windows or fewer kept the pair (whose normalize step then has a
launch of its own).  Unfiltered profiling runs every chunk on one lane.

The burst: the issue's four recordings (5 clip + 3: tail dropped at the aligned hop; 7 samples: one padded window; exactly a clip;
2 clip + min_tail + 1: tail kept, length no multiple of 4) own 16 windows at hop = clip / 2 whatever the clip length, so a fifth,
long recording follows them to bring W above 64: three chunks at max_batch 32, the first one straddling all five recordings.

The stock tiny config's second channel (frame length 256, no FFT form) reads the raw waveform beside the pair, so its plan never
lets PCM go straight into the resident launch (Engine::pcm_direct) and every lane takes k_frame_windows; the tiny geometry with two
FFT-sized channels has the pair alone on the waveform, as the full model does, and is the one that can take the framed form."""
import functools

import numpy as np
import pytest

from birdnet_go_amd import host, synth_model as sm, wav

from test_norm_resident import _names_launched

pytestmark = pytest.mark.gpu

CLIP, HOP, MIN_TAIL, K = 12000, 6000, 7000, 5
LENGTHS = [5 * CLIP + 3, 7, CLIP, 2 * CLIP + MIN_TAIL + 1, 26 * CLIP + 2]


@functools.lru_cache(maxsize=None)
def _fft_tiny_blob():
    spec = sm.SpecConfig(512, 94, 0.0, 3000.0), sm.SpecConfig(512, 94, 500.0, 15000.0)
    return sm.build_model(sm.tiny_config(specs=spec))


def _recordings(lengths, seed=11):
    """int16 material with a level of its own per recording and a few full-scale samples."""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(lengths):
        t = np.arange(n)
        x = (0.2 + 0.1 * i) * np.sin(2 * np.pi * (300.0 + 170.0 * i) * t / 48000.0) + 0.05 * rng.standard_normal(n)
        x[:: max(n // 3, 1)] = -1.0
        out.append(np.clip(np.round(x * 20000.0), -32768, 32767).astype(np.int16))
    return out


def _bytes(pcm16, bits):
    """The same samples at every depth (sample / 2^15 each): 24- and 32-bit are the 16-bit words shifted up, 0 is float32."""
    if bits == 16:
        return pcm16.astype("<i2").tobytes()
    if bits == 0:
        return (pcm16.astype(np.float32) / np.float32(32768.0)).tobytes()
    words = (pcm16.astype(np.int64).reshape(-1) << (bits - 16)).astype("<i4")
    return words.tobytes() if bits == 32 else words.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()


def _host_windows(recs, clip, hop, min_tail):
    """wav.frame_clips' windows of every recording, as int16 (the framing rule does not look at the samples)."""
    rows, owner = [], []
    for r, x in enumerate(recs):
        starts = wav.frame_clips(np.zeros(x.size, np.float32), 1, clip, clip - hop, min_tail)[1].astype(np.int64)
        for j, s0 in enumerate(starts):
            w = np.zeros(clip, np.int16)
            seg = x[s0:s0 + clip]
            w[:seg.size] = seg
            rows.append(w)
            owner.append((r, j))
    return np.stack(rows), owner


def _reference(c, windows, bits, k=K):
    if bits == 0:
        return c.predict_topk(windows.astype(np.float32) / np.float32(32768.0), windows.shape[0], k=k)
    return c.predict_pcm_topk(_bytes(windows.reshape(-1), bits), bits, windows.shape[0], k=k)


def _analyze(c, recs, bits, hop, min_tail=MIN_TAIL, k=K):
    conf, idx, first = c.analyze_pcm_topk(_bytes(np.concatenate(recs), bits), bits, [x.size for x in recs], hop, min_tail, k=k)
    return conf, idx


def _same(got, want):
    assert np.isfinite(got[0]).all()
    assert np.array_equal(got[0], want[0]), np.abs(got[0] - want[0]).max()
    assert np.array_equal(got[1], want[1])


def _profiled(c, call):
    box = {}
    names = _names_launched(c, lambda: box.setdefault("out", call()))
    return box["out"], names


def _minmax_bytes(names):
    return names["clip_minmax"]["bytes"]


@pytest.mark.parametrize("odd", [0, 1])
def test_burst_int16(gpu, odd):
    """hop = clip / 2 and one sample more.  W = 67 (66 at the odd hop): chunks of 32, 32 and 3 (2).  On the two-lane engine every chunk of 32 is two lanes of
    16 (k_frame_windows, then the pair); profiled, and on the one-lane engine, a chunk of 32 is one lane above the 16-window line."""
    hop = HOP + odd
    recs = _recordings(LENGTHS)
    windows, owner = _host_windows(recs, CLIP, hop, MIN_TAIL)
    first = host.analyze_windows(LENGTHS, CLIP, hop, MIN_TAIL)
    W = windows.shape[0]
    assert W == first[-1] and W > 64 and W % 32 <= 16                     # (CPU) three chunks, the last one a small call
    if not odd:
        assert first.tolist() == [0, 9, 10, 11, 16, 67]                   # tail dropped / one padded window / one clip / tail kept
    assert len({r for r, _ in owner[:32]}) == 5                           # the first chunk straddles the recordings
    big, small = W - W % 32, W % 32
    for lanes in (2, 1):
        c = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False, lanes=lanes)
        try:
            assert c.describe()["lanes"] == lanes
            want = _reference(c, windows, 16)
            _same(_analyze(c, recs, 16, hop), want)
            got, names = _profiled(c, lambda: _analyze(c, recs, 16, hop))
            _same(got, want)
            per_sample = 8 if odd else 2 + 4                              # k_frame_windows' floats / the recording's int16
            assert _minmax_bytes(names) == big * CLIP * per_sample + small * CLIP * 4, names["clip_minmax"]
            assert names["clip_minmax"]["launches"] == 3 and names["normalize"]["launches"] == 1, names
        finally:
            c.close()


@pytest.mark.parametrize("bits", [24, 32, 0])
def test_burst_other_depths(gpu, bits):
    """The same burst as packed 24-bit, 32-bit and float32 samples at the aligned hop, one lane: the framed form converts in its load."""
    recs = _recordings(LENGTHS)
    windows, _ = _host_windows(recs, CLIP, HOP, MIN_TAIL)
    c = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False, lanes=1)
    try:
        want = _reference(c, windows, bits)
        _same(want, _reference(c, windows, 16))                           # (the depths carry the same samples)
        _same(_analyze(c, recs, bits, HOP), want)
        got, names = _profiled(c, lambda: _analyze(c, recs, bits, HOP))
        _same(got, want)
        bps = bits // 8 if bits else 4
        assert _minmax_bytes(names) == 64 * CLIP * (bps + 4) + 3 * CLIP * 4, names["clip_minmax"]
    finally:
        c.close()


def test_stock_tiny_plan_frames_first(gpu, tiny_blob):
    """A plan in which another step reads the waveform beside the pair: every chunk goes through k_frame_windows, aligned hop or
    not, and the resident launch (where the lane has more than 16 windows) reads the floats it wrote."""
    recs = _recordings(LENGTHS)
    windows, _ = _host_windows(recs, CLIP, HOP, MIN_TAIL)
    c = host.HipClassifier(tiny_blob, max_batch=32, autotune=False)
    try:
        want = _reference(c, windows, 16)
        _same(_analyze(c, recs, 16, HOP), want)
        got, names = _profiled(c, lambda: _analyze(c, recs, 16, HOP))
        _same(got, want)
        assert _minmax_bytes(names) == 64 * CLIP * 8 + 3 * CLIP * 4, names["clip_minmax"]
    finally:
        c.close()


def test_small_call(gpu):
    """W = 16, the issue's four recordings alone: one lane of 16 windows keeps the small-call min/max behind k_frame_windows."""
    recs = _recordings(LENGTHS[:4])
    windows, _ = _host_windows(recs, CLIP, HOP, MIN_TAIL)
    assert windows.shape[0] == 16
    c = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False)
    try:
        want = _reference(c, windows, 16)
        _same(_analyze(c, recs, 16, HOP), want)
        got, names = _profiled(c, lambda: _analyze(c, recs, 16, HOP))
        _same(got, want)
        assert _minmax_bytes(names) == 16 * CLIP * 4 and names["normalize"]["launches"] == 1, names
    finally:
        c.close()


@pytest.fixture(scope="module")
def full_engine(gpu, full_blob):
    c = host.HipClassifier(full_blob, max_batch=32, autotune=False, lanes=1)
    yield c
    c.close()


def test_full_model_real_offsets(full_engine):
    """144 000-sample windows of one 290 001-sample recording at hop 4 800: 32 windows in one lane, each at an offset of its own into
    the recording - the 28 672 register quads, the LDS part behind them, and a last window of 141 201 valid samples whose final quad
    is partial (the slot's zero fill) and whose tail is zeros inside the LDS part."""
    c = full_engine
    n, hop, mt = 144000, 4800, 48000
    recs = _recordings([290001], seed=5)
    first = host.analyze_windows([290001], n, hop, mt)
    assert first.tolist() == [0, 32]                                      # (CPU) W > 16, one chunk
    windows, owner = _host_windows(recs, n, hop, mt)
    assert windows.shape[0] == 32 and 290001 - owner[-1][1] * hop == 141201
    want = _reference(c, windows, 16)
    _same(_analyze(c, recs, 16, hop, mt), want)
    got, names = _profiled(c, lambda: _analyze(c, recs, 16, hop, mt))
    _same(got, want)
    assert "normalize" not in names and _minmax_bytes(names) == 32 * n * (2 + 4), names["clip_minmax"]


def test_full_model_small_call(full_engine):
    """Four windows of the full model (the last one kept by min_tail 0): k_frame_windows, then the parted small-call min/max (k_clip_minmax_parts) and the pair."""
    c = full_engine
    n, hop = 144000, 72000
    recs = _recordings([2 * n + 11], seed=6)
    windows, _ = _host_windows(recs, n, hop, 0)
    assert windows.shape[0] == 4
    _same(_analyze(c, recs, 16, hop, 0), _reference(c, windows, 16))


def test_detection_rows(gpu):
    """bnhip_analyze_pcm: the rows are the Python filter of the dense result, in window-then-rank order, for a threshold that keeps
    nothing, one that keeps everything, and the exact value of one confidence (kept: >=); a cap below the total writes cap rows
    and still reports the total."""
    recs = _recordings(LENGTHS)
    lengths = [x.size for x in recs]
    raw = _bytes(np.concatenate(recs), 16)
    c = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False)
    try:
        conf, idx, first = c.analyze_pcm_topk(raw, 16, lengths, HOP, MIN_TAIL, k=K)
        W = conf.shape[0]
        rec_of = np.searchsorted(first, np.arange(W), side="right") - 1

        def want_rows(thr):
            rows = [(rec_of[w], w - first[rec_of[w]], idx[w, j], conf[w, j]) for w in range(W) for j in range(K) if conf[w, j] >= thr]
            return np.array(rows, host.DETECTION) if rows else np.zeros(0, host.DETECTION)

        mid = np.float32(np.sort(conf.reshape(-1))[conf.size // 2])
        for thr, count in [(np.float32(2.0), 0), (np.float32(0.0), W * K), (mid, None)]:
            want = want_rows(thr)
            if count is not None:
                assert want.size == count
            else:
                assert 0 < want.size < W * K and (want["confidence"] == mid).any()
            rows, total = c.analyze_pcm(raw, 16, lengths, HOP, MIN_TAIL, k=K, threshold=float(thr))
            assert total == want.size and rows.tobytes() == want.tobytes(), (thr, total, want.size)
        want = want_rows(mid)
        rows, total = c.analyze_pcm(raw, 16, lengths, HOP, MIN_TAIL, k=K, threshold=float(mid), cap=7)
        assert total == want.size > 7 and rows.tobytes() == want[:7].tobytes()
        rows, total = c.analyze_pcm(raw, 16, lengths, HOP, MIN_TAIL, k=K, threshold=float(mid), cap=0)
        assert total == want.size and rows.size == 0
    finally:
        c.close()


def test_refusals_leave_the_handle_usable(gpu):
    """A multi-device handle is refused; a refused call (hop beyond the clip) leaves a single-device handle as it was."""
    recs = _recordings(LENGTHS[:4])
    windows, _ = _host_windows(recs, CLIP, HOP, MIN_TAIL)
    raw, lengths = _bytes(np.concatenate(recs), 16), [x.size for x in recs]
    multi = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False, devices=[0, 0], replicate="peer")
    try:
        with pytest.raises(host.HipError) as ei:
            multi.analyze_pcm_topk(raw, 16, lengths, HOP, MIN_TAIL, k=K)
        assert ei.value.code == host.E_INVALID and "single-device" in str(ei.value)
        with pytest.raises(host.HipError) as ei:
            multi.analyze_pcm(raw, 16, lengths, HOP, MIN_TAIL, k=K)
        assert ei.value.code == host.E_INVALID
    finally:
        multi.close()
    c = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False)
    try:
        want = _reference(c, windows, 16)
        with pytest.raises(host.HipError) as ei:
            c.analyze_pcm_topk(raw, 16, lengths, CLIP + 1, MIN_TAIL, k=K)
        assert ei.value.code == host.E_INVALID
        _same(_analyze(c, recs, 16, HOP), want)
    finally:
        c.close()


def _write_wav16(path, pcm16, rate=48000):
    import struct
    data = pcm16.astype("<i2").tobytes()
    with open(path, "wb") as fh:
        fh.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, rate, rate * 2, 2, 16))
        fh.write(b"data" + struct.pack("<I", len(data)) + data)


def test_analyze_file_device_framing(gpu, tmp_path):
    """wav.analyze_file(device_framing=True) returns the rows of the default path on a 16-bit WAV (half a clip of overlap, a
    threshold that drops rows; 40 windows: two chunks), and analyze_files answers a burst of two files as the two single calls."""
    n = CLIP
    a, b = _recordings([20 * n + n // 2 + 5, 2 * n + 1], seed=3)
    pa, pb = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    _write_wav16(pa, a)
    _write_wav16(pb, b)
    c = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False)
    try:
        rate = 48000
        assert c.n_samples == n
        wa = _host_windows([a], n, n // 2, rate)[0]
        assert wa.shape[0] == 40
        dense = _reference(c, wa, 16)[0]
        thr = float(np.sort(dense.reshape(-1))[dense.size // 3])
        kw = dict(overlap_seconds=n / 2 / rate, top_k=K, threshold=thr, model_rate=rate)
        want = wav.analyze_file(pa, c, **kw)
        got = wav.analyze_file(pa, c, device_framing=True, **kw)
        assert 0 < len(want) < 40 * K and got == want
        both = wav.analyze_files([pa, pb], c, **kw)
        assert both[0] == want and both[1] == wav.analyze_file(pb, c, **kw) and len(both[1]) > 0
    finally:
        c.close()


def test_analyze_file_tawnyowl(full_engine, tmp_path):
    """The committed tawnyowl fixture (32-bit, five clips): the device-framed rows are the default path's."""
    from test_wav import tawnyowl_wav_bytes
    p = str(tmp_path / "tawnyowl.wav")
    with open(p, "wb") as fh:
        fh.write(tawnyowl_wav_bytes())
    want = wav.analyze_file(p, full_engine, top_k=10)
    assert len(want) == 50 and sorted({r[0] for r in want}) == [0.0, 3.0, 6.0, 9.0, 12.0]
    assert wav.analyze_file(p, full_engine, top_k=10, device_framing=True) == want
    thr = sorted(r[3] for r in want)[25]                                  # a confidence of the file itself: kept, and rows below it dropped
    fewer = wav.analyze_file(p, full_engine, top_k=10, threshold=thr)
    assert 0 < len(fewer) < 50 and wav.analyze_file(p, full_engine, top_k=10, threshold=thr, device_framing=True) == fewer
