"""File analysis of multichannel recordings in one device call (bnhip_analyze_channels_pcm_topk / bnhip_analyze_channels_pcm,
bnhip_channel_energy_pcm, wav.analyze_files(channels=...)).

The criterion is bit identity - np.array_equal on conf and idx - with bnhip_analyze_mixed_pcm_topk over the recordings that numpy
builds from the interleaved frames: a channel de-interleaved as it is in the file, or the float32 recording of chanref.mix.  No
tolerance appears: a staged float32 is the same value on both sides (an integer's float32 over a power of two, or one correctly
rounded fp64 division rounded once more), and everything after it is the mixed call's own code.  The 128-bit sums are compared with
Python integers.  The one bound is rms_dbfs, 1e-9 dB: libm's log10 is not correctly rounded, and a few ulp of a value below 100 is
under 1e-13.

The burst is CH_BURST of tests/test_analyze_channels_ref.py, whose length facts are asserted there."""
import ctypes as C
import struct

import numpy as np
import pytest

from birdnet_go_amd import host, wav

import chanref
from test_analyze import _fft_tiny_blob, _profiled, _same
from test_analyze_mixed_ref import CLIP, HOP, K, MIN_TAIL, MODEL_RATE, _bad_tables
from test_analyze_channels_ref import CH_BURST, CH_FIRST, ENERGY_TILE, _bad_channel_tables, ch_recs

pytestmark = pytest.mark.gpu


def _frames(rate, bits, n, channels, rng, levels=None):
    """[n, channels] frames with a tone and noise at a level of its own per channel, and full-scale samples of both signs; integer
    depths carry low bits that a 16-bit word does not have."""
    t = np.arange(n)[:, None]
    c = np.arange(channels)[None, :]
    lv = np.asarray(levels if levels is not None else 0.15 + 0.08 * ((c.reshape(-1) * 5) % 7), np.float64)[None, :]
    x = lv * (np.sin(2 * np.pi * (300.0 + 170.0 * c) * t / rate) + 0.3 * rng.standard_normal((n, channels)))
    if levels is None:
        x[:: max(n // 3, 1), 0] = -1.0
        x[1:: max(n // 2, 2), -1] = 1.0
    if bits == 0:
        return x.astype(np.float32)
    full = 1 << (bits - 1)
    v = np.clip(np.round(x * (full - 1) * 0.9 + (rng.integers(-3, 4, (n, channels)) if levels is None else 0)), -full, full - 1).astype(np.int64)
    v[x == -1.0], v[x == 1.0] = -full, full - 1
    return v


def _mono_bytes(x, bits):
    """A float32 or integer mono recording as the mixed call takes it."""
    return chanref.pack(x.reshape(-1, 1), bits)


@pytest.fixture(scope="module")
def burst(gpu):
    rng = np.random.default_rng(31)
    frames = [_frames(rate, bits, n, ch, rng) for rate, bits, n, ch, _ in CH_BURST]
    return {"frames": frames, "raw": b"".join(chanref.pack(f, b[1]) for f, b in zip(frames, CH_BURST))}


@pytest.fixture(scope="module")
def engine(gpu, burst):
    """The two-lane engine and, computed once, what the mixed call answers for the burst's fixed channels and for its mixes."""
    c = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False, lanes=2)
    yield c, {"fixed": _want_fixed(c, burst), "mix": _want_mix(c, burst)}
    c.close()


def _want_fixed(c, burst, hop=HOP):
    """analyze_mixed_pcm_topk over every recording's channel, de-interleaved in numpy and kept at its own depth."""
    raw = b"".join(_mono_bytes(f[:, b[4]], b[1]) for f, b in zip(burst["frames"], CH_BURST))
    recs = host.recordings([b[2] for b in CH_BURST], [b[0] for b in CH_BURST], [b[1] for b in CH_BURST])
    return c.analyze_mixed_pcm_topk(raw, recs, MODEL_RATE, hop, MIN_TAIL, k=K)


def _want_mix(c, burst, hop=HOP):
    """... and over the float32 recordings of chanref.mix."""
    raw = b"".join(chanref.mix(f, b[1]).tobytes() for f, b in zip(burst["frames"], CH_BURST))
    recs = host.recordings([b[2] for b in CH_BURST], [b[0] for b in CH_BURST], 0)
    return c.analyze_mixed_pcm_topk(raw, recs, MODEL_RATE, hop, MIN_TAIL, k=K)


def _check_burst(c, burst, select, want, hop=HOP):
    conf, idx, first, chosen = c.analyze_channels_pcm_topk(burst["raw"], ch_recs(select=select), MODEL_RATE, hop, MIN_TAIL, k=K)
    assert np.array_equal(first, want[2])
    _same((conf, idx), want[:2])
    return chosen


def test_fixed_channel(engine, burst):
    """All four depths, 1 / 2 / 3 / 4 / 8 channels, rates at and off the model's; lanes 2 and 1, and an odd hop."""
    c2, want = engine
    assert want["fixed"][2].tolist() == CH_FIRST and want["fixed"][0].shape == (CH_FIRST[-1], K)
    chosen = _check_burst(c2, burst, None, want["fixed"])
    assert chosen.tolist() == [b[4] for b in CH_BURST]
    one = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False, lanes=1)
    try:
        _check_burst(one, burst, None, _want_fixed(one, burst))
    finally:
        one.close()
    _check_burst(c2, burst, None, _want_fixed(c2, burst, HOP + 1), HOP + 1)
    # another channel of the same frames answers other rows (the test would not see a launch that always read channel 0)
    other = c2.analyze_channels_pcm_topk(burst["raw"], ch_recs(select=0), MODEL_RATE, HOP, MIN_TAIL, k=K)
    assert not np.array_equal(other[0], want["fixed"][0])


def test_mix(engine, burst):
    c2, want = engine
    chosen = _check_burst(c2, burst, "mix", want["mix"])
    assert (chosen == host.CHANNEL_MIX).all()
    one = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False, lanes=1)
    try:
        _check_burst(one, burst, "mix", _want_mix(one, burst))
    finally:
        one.close()
    _check_burst(c2, burst, "mix", _want_mix(c2, burst, HOP + 1), HOP + 1)


# (rate, bits, frames, per-channel levels): left 12 dB up, right 12 dB up, within 3 dB, both below -60 dBFS, four channels with the
# loudest on index 2.  Frame counts that leave a ragged end behind the last 16-byte vector and cross a measurement tile.
_AUTO = [(44100, 16, 2 * ENERGY_TILE + 4099, [0.4, 0.1]), (48000, 24, ENERGY_TILE + 15001, [0.05, 0.2]), (32000, 32, 9003, [0.2, 0.15]),
         (48000, 16, 12001, [0.0006, 0.0002]), (96000, 16, 30001, [0.04, 0.05, 0.2, 0.03])]
_AUTO_WANT = [0, 1, chanref.MIX, chanref.MIX, 2]


@pytest.fixture(scope="module")
def auto_burst(gpu):
    rng = np.random.default_rng(47)
    frames = [_frames(rate, bits, n, len(lv), rng, levels=lv) for rate, bits, n, lv in _AUTO]
    rows = [(rate, bits, n, len(lv), 0) for rate, bits, n, lv in _AUTO]
    energy = [chanref.energies(f) for f in frames]
    return {"frames": frames, "rows": rows, "energy": energy, "raw": b"".join(chanref.pack(f, r[1]) for f, r in zip(frames, rows))}


def test_auto(engine, auto_burst):
    c, _ = engine
    rows, frames, raw = auto_burst["rows"], auto_burst["frames"], auto_burst["raw"]
    want_sel = [chanref.decide(e, r[1], r[2]) for e, r in zip(auto_burst["energy"], rows)]
    assert want_sel == _AUTO_WANT                                          # (CPU) the cases are what the table says
    got = c.analyze_channels_pcm_topk(raw, ch_recs(rows, "auto"), MODEL_RATE, HOP, MIN_TAIL, k=K)
    assert got[3].tolist() == want_sel
    # the rows of the corresponding fixed / mix call, and of the mixed call over what numpy picks
    same = c.analyze_channels_pcm_topk(raw, ch_recs(rows, want_sel), MODEL_RATE, HOP, MIN_TAIL, k=K)
    _same(got[:2], same[:2])
    assert same[3].tolist() == want_sel
    picked = [chanref.pick(f, r[1], s) for f, r, s in zip(frames, rows, want_sel)]
    want = c.analyze_mixed_pcm_topk(b"".join(p.tobytes() for p in picked), host.recordings([r[2] for r in rows], [r[0] for r in rows], 0),
                                    MODEL_RATE, HOP, MIN_TAIL, k=K)
    assert np.array_equal(got[2], want[2])
    _same(got[:2], want[:2])
    # a burst that mixes the three kinds of selection: only its auto recordings are measured
    sel = ["auto", 0, "mix", "auto", 3]
    mixed_sel = c.analyze_channels_pcm_topk(raw, ch_recs(rows, sel), MODEL_RATE, HOP, MIN_TAIL, k=K)
    assert mixed_sel[3].tolist() == [want_sel[0], 0, chanref.MIX, want_sel[3], 3]
    # the measurement alone
    energy, chosen = host.channel_energy(raw, ch_recs(rows, 0))
    assert chosen.tolist() == want_sel
    flat = [(e, r) for es, r in zip(auto_burst["energy"], rows) for e in es]
    assert len(energy) == len(flat) == 12
    for got_e, (e, r) in zip(energy, flat):
        assert (int(got_e["sum_lo"]), int(got_e["sum_hi"])) == chanref.split128(e)
        assert abs(float(got_e["rms_dbfs"]) - chanref.rms_dbfs(e, r[1], r[2])) <= 1e-9
    assert energy["rms_dbfs"][6] < -60.0 and energy["rms_dbfs"][7] < -60.0 and energy["sum_hi"][:2].tolist() == [0, 0]


def test_carries(gpu):
    """32-bit recordings with runs of -2^31 (five such squares pass 2^64), on the vector form (2 channels) and the sample form (3
    channels), three measurement tiles each: the 128-bit sums are exact, wherever the recording sits in the burst."""
    rng = np.random.default_rng(5)
    recs, frames = [], []
    for n, ch in ((2 * ENERGY_TILE + 7001, 2), (2 * ENERGY_TILE + 1 + 2047, 3), (1000, 2)):
        v = rng.integers(-(1 << 31), 1 << 31, (n, ch), dtype=np.int64)
        for start, stop in ((0, 700), (ENERGY_TILE - 300, ENERGY_TILE + 300), (n - 64, n)):        # a thread's, a wave's, a block's and a tile's edge
            v[start:stop, 0] = -(1 << 31)
        v[5000:5900, ch - 1] = -(1 << 31)
        recs.append((48000, 32, n, ch, 0))
        frames.append(v)
    want = [chanref.energies(f) for f in frames]
    assert all(e[0] >> 64 > 0 for e in want) and sum(1 for f in frames if f.shape[0] > 2 * ENERGY_TILE) == 2
    for order in ([0, 1, 2], [2, 1, 0]):
        energy, chosen = host.channel_energy(b"".join(chanref.pack(frames[i], 32) for i in order), ch_recs([recs[i] for i in order], 0))
        got = [(int(e["sum_lo"]), int(e["sum_hi"])) for e in energy]
        assert got == [chanref.split128(e) for i in order for e in want[i]], order
        assert chosen.tolist() == [chanref.decide(want[i], 32, recs[i][2]) for i in order]


def test_fast_path_is_the_mixed_call(engine, burst):
    """An all-mono burst: the launch names and counts of bnhip_analyze_mixed_pcm_topk, read from the per-step profile; a multichannel
    burst without auto shows the same steps again (the profile rows are the engine's steps: neither the slot launch nor a
    measurement is among them, and the chunks are launched as they were)."""
    c, _ = engine
    mono = [(b[0], b[1], b[2], 1, 0) for b in CH_BURST]
    raw = b"".join(_mono_bytes(f[:, 0], b[1]) for f, b in zip(burst["frames"], CH_BURST))
    recs = host.recordings([b[2] for b in mono], [b[0] for b in mono], [b[1] for b in mono])
    want, names_want = _profiled(c, lambda: c.analyze_mixed_pcm_topk(raw, recs, MODEL_RATE, HOP, MIN_TAIL, k=K))
    for select, chosen_want in ((0, 0), ("mix", host.CHANNEL_MIX)):
        got, names = _profiled(c, lambda: c.analyze_channels_pcm_topk(raw, ch_recs(mono, select), MODEL_RATE, HOP, MIN_TAIL, k=K))
        _same(got[:2], want[:2])
        assert np.array_equal(got[2], want[2]) and (got[3] == chosen_want).all()
        assert {n: (v["launches"], v["bytes"]) for n, v in names.items()} == {n: (v["launches"], v["bytes"]) for n, v in names_want.items()}
    # int16 mono at the model's rate: the existing call's own fast path (no float32 slots, no resample launch)
    plain = [(MODEL_RATE, 16, b[2], 1, 0) for b in CH_BURST[:4]]
    assert all(b[1] >= 16 for b in CH_BURST[:4])
    praw = b"".join(_mono_bytes(f[:, 0] >> (b[1] - 16), 16) for f, b in zip(burst["frames"], CH_BURST[:4]))
    want, names_want = _profiled(c, lambda: c.analyze_pcm_topk(praw, 16, [b[2] for b in plain], HOP, MIN_TAIL, k=K))
    got, names = _profiled(c, lambda: c.analyze_channels_pcm_topk(praw, ch_recs(plain, "auto"), MODEL_RATE, HOP, MIN_TAIL, k=K))
    _same(got[:2], want[:2])
    assert (got[3] == 0).all()
    assert {n: (v["launches"], v["bytes"]) for n, v in names.items()} == {n: (v["launches"], v["bytes"]) for n, v in names_want.items()}
    got, names = _profiled(c, lambda: c.analyze_channels_pcm_topk(burst["raw"], ch_recs(), MODEL_RATE, HOP, MIN_TAIL, k=K))
    assert not [n for n in names if "energy" in n or "decide" in n]


def test_detection_rows(engine, burst):
    """bnhip_analyze_channels_pcm's rows are bnhip_analyze_mixed_pcm's over the de-interleaved channels, byte for byte, for a threshold
    that keeps some rows and drops some; a cap below the total writes cap rows and reports the total; cap 0 takes out = NULL."""
    c, want = engine
    raw = b"".join(_mono_bytes(f[:, b[4]], b[1]) for f, b in zip(burst["frames"], CH_BURST))
    recs = host.recordings([b[2] for b in CH_BURST], [b[0] for b in CH_BURST], [b[1] for b in CH_BURST])
    conf = want["fixed"][0]
    mid = float(np.sort(conf.reshape(-1))[conf.size // 2])
    want_rows, want_total = c.analyze_mixed_pcm(raw, recs, MODEL_RATE, HOP, MIN_TAIL, k=K, threshold=mid)
    assert 0 < want_total < conf.size and want_rows.size == want_total and len(set(want_rows["recording"].tolist())) > 1
    rows, total, chosen = c.analyze_channels_pcm(burst["raw"], ch_recs(), MODEL_RATE, HOP, MIN_TAIL, k=K, threshold=mid)
    assert total == want_total and rows.tobytes() == want_rows.tobytes() and chosen.tolist() == [b[4] for b in CH_BURST]
    rows, total, _ = c.analyze_channels_pcm(burst["raw"], ch_recs(), MODEL_RATE, HOP, MIN_TAIL, k=K, threshold=mid, cap=7)
    assert total == want_total > 7 and rows.tobytes() == want_rows[:7].tobytes()
    rows, total, _ = c.analyze_channels_pcm(burst["raw"], ch_recs(), MODEL_RATE, HOP, MIN_TAIL, k=K, threshold=mid, cap=0)
    assert total == want_total and rows.size == 0


def test_refusals_leave_the_handle_usable(engine, burst):
    """Every refusal of the list on a live handle: BNHIP_E_INVALID with nothing written; a multi-device handle is refused; the handle
    then answers the fixed-channel burst as before."""
    c, want = engine
    lib = host._analyze_channels_protos(c._lib)
    some = np.zeros(64, np.uint8)
    conf, idx = np.full((8, K), -7, np.float32), np.full((8, K), -7, np.int32)
    det, n_det, chosen = np.zeros(8, host.DETECTION), C.c_size_t(12345), np.full(40, -7, np.int32)
    energy = np.zeros(64, host.CHANNEL_ENERGY)
    energy["rms_dbfs"] = -7.0
    P = lambda a: a.ctypes.data
    tables = [(what, bad, MODEL_RATE) for what, bad in _bad_channel_tables()]
    tables += [(what, host.channel_recordings(bad["length"], bad["rate"], bad["bits_per_sample"], 2, 1), rate) for what, bad, rate in _bad_tables()]
    for what, bad, rate in tables:
        assert lib.bnhip_analyze_channels_pcm_topk(c._h, P(some), P(bad), len(bad), rate, HOP, MIN_TAIL, 0, 1.0, K, P(conf), P(idx),
                                                   P(chosen)) == host.E_INVALID, what
        assert lib.bnhip_analyze_channels_pcm(c._h, P(some), P(bad), len(bad), rate, HOP, MIN_TAIL, 0, 1.0, K, 0.0, P(det), 8, C.byref(n_det),
                                              P(chosen)) == host.E_INVALID, what
    for what, bad in _bad_channel_tables():
        assert lib.bnhip_channel_energy_pcm(0, P(some), P(bad), len(bad), P(energy), P(chosen)) == host.E_INVALID, what
    recs = ch_recs()
    for null in ("h", "pcm", "recs", "out"):
        assert lib.bnhip_analyze_channels_pcm_topk(None if null == "h" else c._h, None if null == "pcm" else P(some), None if null == "recs" else P(recs),
                                                   len(recs), MODEL_RATE, HOP, MIN_TAIL, 0, 1.0, K, None if null == "out" else P(conf), P(idx),
                                                   P(chosen)) == host.E_INVALID, null
    for nr in (0, 65536):
        assert lib.bnhip_analyze_channels_pcm_topk(c._h, P(some), P(recs), nr, MODEL_RATE, HOP, MIN_TAIL, 0, 1.0, K, P(conf), P(idx),
                                                   P(chosen)) == host.E_INVALID
    assert (conf == -7).all() and (idx == -7).all() and not det["confidence"].any() and n_det.value == 12345
    assert (chosen == -7).all() and (energy["rms_dbfs"] == -7.0).all()
    for kw in [dict(hop=0), dict(hop=CLIP + 1), dict(min_tail=-1), dict(k=0), dict(activation=3)]:
        args = dict(hop=HOP, min_tail=MIN_TAIL, k=K)
        args.update(kw)
        for call in (c.analyze_channels_pcm_topk, c.analyze_channels_pcm):
            with pytest.raises(host.HipError) as ei:
                call(burst["raw"], recs, MODEL_RATE, **args)
            assert ei.value.code == host.E_INVALID, kw
    multi = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False, devices=[0, 0], replicate="peer")
    try:
        with pytest.raises(host.HipError) as ei:
            multi.analyze_channels_pcm_topk(burst["raw"], recs, MODEL_RATE, HOP, MIN_TAIL, k=K)
        assert ei.value.code == host.E_INVALID and "single-device" in str(ei.value)
    finally:
        multi.close()
    _check_burst(c, burst, None, want["fixed"])


def _wav_bytes(raw, rate, bits, channels):
    return (b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, channels, rate, rate * channels * bits // 8,
                                                                                        channels * bits // 8, bits)
            + b"data" + struct.pack("<I", len(raw)) + raw)


def test_analyze_files_channels(gpu, tmp_path):
    """wav.analyze_files(channels=0) is today's first-channel path; "mix" and "auto" are the direct calls; analyze_file passes the
    keywords through."""
    rng = np.random.default_rng(9)
    files = [(44100, 16, 30001, [0.3, 0.05]), (96000, 24, 50003, [0.1, 0.12, 0.11, 0.09]), (48000, 16, 2 * CLIP + 9000, [0.05, 0.3]),
             (48000, 16, 13000, [0.2])]
    paths, frames = [], []
    for i, (rate, bits, n, lv) in enumerate(files):
        frames.append(_frames(rate, bits, n, len(lv), rng, levels=lv))
        paths.append(str(tmp_path / f"{i}.wav"))
        with open(paths[-1], "wb") as fh:
            fh.write(_wav_bytes(chanref.pack(frames[-1], bits), rate, bits, len(lv)))
        data, got_rate, got_bits, got_ch = wav.read_wav_frames(paths[-1])
        assert (got_rate, got_bits, got_ch) == (rate, bits, len(lv)) and data == chanref.pack(frames[-1], bits)
    c = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False)
    try:
        kw = dict(overlap_seconds=CLIP / 2 / MODEL_RATE, top_k=K, model_rate=MODEL_RATE)
        dense = wav.analyze_files(paths, c, **kw)
        thr = sorted(r[3] for rows in dense for r in rows)[sum(len(rows) for rows in dense) // 3]
        want = wav.analyze_files(paths, c, threshold=thr, **kw)
        assert 0 < sum(len(w) for w in want) < sum(len(d) for d in dense)
        assert wav.analyze_files(paths, c, threshold=thr, channels=0, **kw) == want
        assert wav.analyze_files(paths, c, threshold=thr, device_resample=True, **kw) == want
        got, chosen = wav.analyze_files(paths, c, threshold=thr, channels=0, return_chosen=True, **kw)
        assert got == want and chosen == [0, 0, 0, 0]
        assert wav.analyze_file(paths[1], c, threshold=thr, channels=0, **kw) == want[1]
        # "mix" / "auto": the rows of the direct call over the same frames, turned into rows as analyze_files turns them
        raw = b"".join(chanref.pack(f, r[1]) for f, r in zip(frames, files))
        hop = CLIP - CLIP // 2
        for choice, want_chosen in (("mix", ["mix"] * 4), ("auto", [0, "mix", 1, 0])):
            recs = host.channel_recordings([r[2] for r in files], [r[0] for r in files], [r[1] for r in files], [len(r[3]) for r in files], choice)
            det, _, sel = c.analyze_channels_pcm(raw, recs, MODEL_RATE, hop, MODEL_RATE, k=K, threshold=float(np.float32(0.0)))
            direct = [[] for _ in files]
            for r, w, j, cf in zip(det["recording"], det["window"], det["class_index"], det["confidence"]):
                start = np.float64(int(w) * hop) / MODEL_RATE
                direct[int(r)].append((float(start), float(start + CLIP / float(MODEL_RATE)), int(j), float(cf)))
            got, chosen = wav.analyze_files(paths, c, channels=choice, return_chosen=True, **kw)
            assert got == direct and chosen == want_chosen == ["mix" if s < 0 else int(s) for s in sel]
            rows1, chosen1 = wav.analyze_file(paths[2], c, channels=choice, return_chosen=True, **kw)
            assert rows1 == direct[2] and chosen1 == want_chosen[2]
    finally:
        c.close()
