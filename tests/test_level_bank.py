"""The audio level bank on the device against the restatement (tests/levelref.py): exact integers and levels for every frame
length class and bit depth, 64-bit sums, frame edges, the same bytes on every run, the bank's state, every refusal, the capture
write that also measures, and WindowBatcher.set_audio_level on the tiny model with native and Python rings."""
import ctypes as C

import numpy as np
import pytest

from birdnet_go_amd import host

import levelref

pytestmark = pytest.mark.gpu

# the smallest lengths at which the tile search (tiles of 8192 / 4096 samples), the ragged last 16-byte line, the cross-wave
# reduction (more than 64 lanes of a block at work from 513 samples on) and several tiles of one frame can each go wrong
LENGTHS = [0, 1, 7, 8, 9, 2047, 2048, 2049, 4097, 70001]
STREAM_OF = [0, 1, 2, 1, 3, 1, 4, 0, 2, 3]                # stream 1 is listed three times


def _pcm(rng, n, bits):
    """n samples of `bits` as bytes: noise with full-scale values in it, and for 24 / 32 bit the values that decide the rounding."""
    if bits == 16:
        v = rng.integers(-32768, 32768, n).astype("<i2")
        if n > 100:
            v[rng.integers(0, n, 5)] = [32767, -32768, 32767, 32766, -32767]
        return v.tobytes()
    if bits == 32:
        v = rng.integers(-2 ** 31, 2 ** 31, n).astype("<i4")
        edge = np.array([0x8000, 0x18000, -0x8000, -0x18000, 0x7FFFFFFF, -0x80000000, 0x7FFF8000, 0x7FFF7FFF], np.int64).astype("<i4")
        v[:min(n, edge.size)] = edge[:n]
        return v.tobytes()
    v = rng.integers(-2 ** 23, 2 ** 23, n).astype(np.int32)
    edge = np.array([0x80, 0x180, 0x280, -0x80, -0x180, 0x7FFFFF, -0x800000, 0x7FFF7F, 0x7FFF80], np.int32)
    v[:min(n, edge.size)] = edge[:n]
    return np.stack([(v >> s) & 0xFF for s in (0, 8, 16)], 1).astype(np.uint8).tobytes()


def _want(frames, bits=16):
    """[(stream, bytes)] -> the records the restatement gives, as tuples (stream, frame, level, clipping, n, clipped, sum)."""
    out = []
    for f, (st, raw) in enumerate(frames):
        q = levelref.pcm16_of(raw, bits)
        total, clipped, level, clipping = levelref.measure(q)
        out.append((st, f, level, int(clipping), q.size, clipped, total))
    return out


def _got(recs):
    return [tuple(int(r[k]) for k in ("stream", "frame", "level", "clipping", "n_samples", "clipped_samples", "sum_squares")) for r in recs]


@pytest.fixture()
def bank(gpu):
    b = host.LevelBank(max_streams=8)
    for _ in range(5):
        b.add_stream()
    yield b
    b.close()


@pytest.mark.parametrize("bits", [16, 24, 32])
def test_every_record_is_exact(bank, bits):
    rng = np.random.default_rng(bits)
    frames = [(st, _pcm(rng, n, bits)) for st, n in zip(STREAM_OF, LENGTHS)]
    want = _want(frames, bits)
    assert sum(w[3] for w in want) >= 1 and any(w[5] == 0 for w in want if w[4] >= 1)     # clipping and clean frames both occur
    assert _got(bank.process(frames, bits)) == want


def test_sums_are_64_bit_at_lane_wave_and_block_level(bank):
    n = 65539
    rec = bank.process([(0, np.full(n, -32768, np.int16))])[0]
    assert int(rec["sum_squares"]) == n << 30 and int(rec["clipped_samples"]) == n and int(rec["level"]) == 100
    # one 16-byte line alone already passes 2^32, one wave 2^38
    rec = bank.process([(0, np.full(8, -32768, np.int16)), (1, np.full(512, 32767, np.int16))])
    assert int(rec[0]["sum_squares"]) == 8 << 30 and int(rec[1]["sum_squares"]) == 512 * 32767 * 32767


@pytest.mark.parametrize("n_first", [3, 8, 13, 2049])
def test_a_frame_never_reads_its_neighbour(bank, n_first):
    """Adjacent frames: a full-scale sample as the last of the first frame, then as the very first of the second, does not reach the
    other frame's record."""
    quiet = np.full(21, 5, np.int16)
    first = np.full(n_first, 5, np.int16)
    first[-1] = 32767
    rec = bank.process([(0, first), (1, quiet)])
    assert int(rec[1]["clipping"]) == 0 and int(rec[1]["sum_squares"]) == 21 * 25 and int(rec[0]["clipped_samples"]) == 1
    second = quiet.copy()
    second[0] = 32767
    calm = np.full(n_first, 5, np.int16)
    rec = bank.process([(0, calm), (1, second)])
    assert int(rec[0]["clipping"]) == 0 and int(rec[0]["sum_squares"]) == n_first * 25
    assert int(rec[1]["clipped_samples"]) == 1 and int(rec[1]["sum_squares"]) == 20 * 25 + 32767 * 32767 and int(rec[1]["level"]) == 95


def test_odd_byte_counts(bank):
    raw = np.full(5, 1000, "<i2").tobytes() + b"\x7f"
    rec = bank.process([(0, raw)])[0]                                   # 16 bit: the last byte is dropped, as the reference truncates
    assert int(rec["n_samples"]) == 5 and int(rec["sum_squares"]) == 5 * 1000 * 1000
    for bits in (24, 32):
        with pytest.raises(host.HipError) as e:
            bank.process([(0, b"\0" * 7)], bits)
        assert e.value.code == host.E_INVALID


def test_the_same_call_gives_the_same_bytes(bank):
    rng = np.random.default_rng(5)
    frames = [(st, _pcm(rng, n, 16)) for st, n in zip(STREAM_OF, LENGTHS)]
    a = bank.process(frames).tobytes()
    assert bank.process(frames).tobytes() == a


def test_latest_and_stats_follow_the_restatement(gpu):
    bank = host.LevelBank(max_streams=4)
    s0, s1, s2 = bank.add_stream(), bank.add_stream(), bank.add_stream()
    rng = np.random.default_rng(9)
    ref = {s: levelref.Stats() for s in (s0, s1, s2)}
    last = {}

    def call(frames):
        recs = bank.process(frames)
        want = _want(frames)
        assert _got(recs) == want
        for w in want:
            ref[w[0]].record(w[2], w[3])
            last[w[0]] = w

    assert (bank.latest()["stream"] == -1).all() and bank.stats(s0) == levelref.Stats().fields()
    amp = lambda a, n: (rng.integers(-a, a + 1, n)).astype("<i2").tobytes()
    call([(s0, amp(20, 900)), (s1, amp(3000, 777)), (s0, b""), (s0, amp(32767, 5000))])
    call([(s1, amp(200, 4097)), (s0, np.zeros(480, np.int16).tobytes())])
    call([(s0, amp(9000, 33)), (s1, np.full(100, 32767, np.int16).tobytes()), (s1, amp(60, 60))])
    lat = bank.latest()
    assert _got(lat[[s0, s1]]) == [last[s0], last[s1]] and int(lat[s2]["stream"]) == -1 and int(lat[3]["stream"]) == -1
    assert ref[s0].zero_count >= 2 and ref[s1].clip_count >= 1                  # the sequence has zeros and clipping frames
    assert bank.stats(s0) == ref[s0].fields() and bank.stats(s2) == ref[s2].fields()
    assert bank.stats(s1, reset=True) == ref[s1].fields()
    ref[s1] = levelref.Stats()
    assert bank.stats(s1) == ref[s1].fields() and _got(bank.latest()[[s1]]) == [last[s1]]      # logAndReset: the summary starts again
    call([(s1, amp(500, 50))])
    assert bank.stats(s1) == ref[s1].fields() and bank.stats(s1)["count"] == 1
    bank.remove_stream(s0)                                                       # a reused slot starts fresh
    assert int(bank.latest()[s0]["stream"]) == -1
    assert bank.add_stream() == s0
    ref[s0] = levelref.Stats()
    assert bank.stats(s0) == ref[s0].fields() and int(bank.latest()[s0]["stream"]) == -1
    call([(s0, amp(100, 10)), (s2, amp(100, 10))])
    bank.reset(s2)
    assert bank.stats(s2) == levelref.Stats().fields() and int(bank.latest()[s2]["stream"]) == -1 and bank.stats(s0)["count"] == 1
    bank.reset(-1)
    assert (bank.latest()["stream"] == -1).all() and all(bank.stats(s) == levelref.Stats().fields() for s in (s0, s1, s2))
    bank.close()


def test_refusals_leave_the_handle_usable(gpu):
    lib = host.load_library()
    rng = np.random.default_rng(3)
    bank = host.LevelBank(max_streams=4)
    s0, s1 = bank.add_stream(), bank.add_stream()
    gone = bank.add_stream()
    bank.remove_stream(gone)
    good = [(s0, _pcm(rng, 3000, 16)), (s1, _pcm(rng, 17, 16))]
    h = bank._alive()
    x = np.zeros(16, np.int16)
    out = np.zeros(4, host.AUDIO_LEVEL)
    alive = []                                                          # the arrays whose addresses the calls below pass

    def arr(dtype, *v):
        alive.append(np.array(v, dtype))
        return alive[-1].ctypes.data

    i32, i64 = (lambda *v: arr(np.int32, *v)), (lambda *v: arr(np.int64, *v))
    ptrs = lambda *v: (C.c_void_p * len(v))(*v)

    def refused():
        P = lib.bnhip_level_bank_process_pcm
        st, n, p, o = i32(s0), i64(16), ptrs(x.ctypes.data), out.ctypes.data
        calls = [
            (None, 1, st, n, p, 16, o),                       # NULL where a pointer is required
            (h, 1, None, n, p, 16, o), (h, 1, st, None, p, 16, o),
            (h, 1, st, n, None, 16, o), (h, 1, st, n, p, 16, None),
            (h, -1, st, n, p, 16, o),
            (h, 1, st, n, p, 8, o), (h, 1, st, n, p, 20, o),   # bits
            (h, 1, i32(3), n, p, 16, o),                      # a stream never added
            (h, 1, i32(gone), n, p, 16, o),                   # a removed stream
            (h, 1, i32(-1), n, p, 16, o), (h, 1, i32(4), n, p, 16, o),
            (h, 1, st, i64(-1), p, 16, o),                    # a negative length
            (h, 1, st, i64((1 << 23) + 1), p, 16, o),         # a frame above 2^23 samples
            (h, 1, st, n, ptrs(None), 16, o),                 # a NULL frame of non-zero length
        ]
        for a in calls:
            assert P(*a) == host.E_INVALID, a
        # a total of 2^36 samples or more: 2^13 frames of 2^23 (checked before any frame is read)
        k = 1 << 13
        many = np.zeros(k, host.AUDIO_LEVEL)
        assert P(h, k, i32(*[s0] * k), i64(*[1 << 23] * k), (C.c_void_p * k)(*[x.ctypes.data] * k), 16, many.ctypes.data) == host.E_INVALID
        assert lib.bnhip_level_bank_latest(h, None) == host.E_INVALID and lib.bnhip_level_bank_stats(h, s0, 0, None) == host.E_INVALID
        assert lib.bnhip_level_bank_stats(h, gone, 0, o) == host.E_INVALID
        assert lib.bnhip_level_bank_reset(h, gone) == host.E_INVALID and lib.bnhip_level_bank_reset(h, -2) == host.E_INVALID
        assert lib.bnhip_level_bank_remove_stream(h, gone) == host.E_INVALID
        s = C.c_int()
        assert lib.bnhip_level_bank_add_stream(h, None) == host.E_INVALID and lib.bnhip_level_bank_add_stream(None, C.byref(s)) == host.E_INVALID
        hh = C.c_void_p()
        for bad in (0, 65536):
            assert lib.bnhip_level_bank_create(0, bad, C.byref(hh)) == host.E_INVALID
        assert lib.bnhip_level_bank_create(0, 4, None) == host.E_INVALID

    refused()                                                                                       # before any good call
    first = bank.process(good)
    assert _got(first) == _want(good)
    state = (bank.latest().tobytes(), bank.stats(s0), bank.stats(s1))
    refused()
    assert (bank.latest().tobytes(), bank.stats(s0), bank.stats(s1)) == state                      # a refusal changes nothing
    assert bank.process(good).tobytes() == first.tobytes()                                          # and the handle answers identically
    full = host.LevelBank(max_streams=1)
    full.add_stream()
    with pytest.raises(host.HipError) as e:
        full.add_stream()
    assert e.value.code == host.E_INVALID
    full.close()
    bank.close()


# ------------------------------------------------------------------------------------------ the capture write that also measures
@pytest.mark.parametrize("bits", [16, 24])
def test_fused_write_stores_as_write_and_measures_as_process(gpu, bits):
    cap, n_src = 4096, 8
    rng = np.random.default_rng(40 + bits)
    fused, twin = host.CaptureBank(n_src, 0, 48000, capacity_samples=cap), host.CaptureBank(n_src, 0, 48000, capacity_samples=cap)
    lv, lv_alone = host.LevelBank(8), host.LevelBank(8)
    for _ in range(n_src):
        assert lv.add_stream() == lv_alone.add_stream()
    calls = [
        # unaligned lengths; source 2 three times
        [(0, 1001), (1, 7), (2, 2049), (3, 0), (2, 13), (4, 3333), (2, 1), (7, 4095)],
        # source 0 and 2 wrap their rings; source 5's frames total more than its ring (4097 + 1000 + 2000 > 4096): stored trimmed,
        # measured in full
        [(0, 3500), (5, 4097), (2, 2500), (5, 1000), (6, 9), (5, 2000), (1, 4090)],
    ]
    for k, call in enumerate(calls):
        frames = [(s, _pcm(rng, n, bits)) for s, n in call]
        streams = [s if (k, i) not in ((0, 4), (1, 4)) else -1 for i, (s, _) in enumerate(frames)]      # one frame per call is not measured
        before = lv.latest().tobytes(), [lv.stats(s) for s in range(n_src)]
        recs = fused.write(frames, bits, levels=(lv, streams))
        assert twin.write(frames, bits) is None
        measured = [(st, f) for st, (_, f) in zip(streams, frames) if st >= 0]
        alone = lv_alone.process(measured, bits)
        keep = [i for i, st in enumerate(streams) if st >= 0]
        cols = ["stream", "level", "clipping", "n_samples", "clipped_samples", "sum_squares"]
        for c in cols:
            assert np.array_equal(recs[keep][c], alone[c]), c
        assert [int(v) for v in recs[keep]["frame"]] == keep
        skipped = [i for i, st in enumerate(streams) if st < 0]
        assert len(skipped) == 1 and int(recs[skipped[0]]["stream"]) == -1 and int(recs[skipped[0]]["sum_squares"]) == 0
        assert _got(recs[keep]) == [w for w in _want([(st if st >= 0 else 0, f) for st, (_, f) in zip(streams, frames)], bits) if w[1] in keep]
        assert lv.latest().tobytes() != before[0]
        untouched = [s for s in range(n_src) if s not in {st for st in streams if st >= 0}]
        assert untouched and all(lv.stats(s) == before[1][s] for s in untouched)
        # the rings and the clocks are those of the plain write
        a, b = fused.positions(), twin.positions()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        spans = np.zeros(n_src, host.CLIP_SPAN)
        for s in range(n_src):
            spans[s] = (int(a[1][s]), int(a[0][s] - a[1][s]), s)
        got, want = fused.read(spans), twin.read(spans)
        assert len(got) == len(want) >= 5 and all(np.array_equal(g, w) for g, w in zip(got, want))
    for c in cols:                                                      # (`frame` counts the call's frames, measured or not)
        assert np.array_equal(lv.latest()[c], lv_alone.latest()[c]), c
    assert all(lv.stats(s) == lv_alone.stats(s) for s in range(n_src))
    # refusals of either bank come before any device work and change neither
    state = fused.positions(), lv.latest().tobytes()
    x = _pcm(rng, 10, bits)
    for frames, streams in ([(0, x)], [99]), ([(8, x)], [0]), ([(0, x)], [-2]):
        with pytest.raises(host.HipError) as e:
            fused.write(frames, bits, levels=(lv, streams))
        assert e.value.code == host.E_INVALID
    after = fused.positions()
    assert np.array_equal(after[0], state[0][0]) and np.array_equal(after[1], state[0][1]) and lv.latest().tobytes() == state[1]
    for b in (fused, twin, lv, lv_alone):
        b.close()


# ------------------------------------------------------------------------------------------ WindowBatcher.set_audio_level
@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
def test_window_batcher_audio_levels(gpu, tiny_cfg, tiny_blob, native):
    from birdnet_go_amd import results as R, stream as S
    clf = host.HipClassifier(tiny_blob, device=0, max_batch=8)
    bn = host.BirdNET(clf, [f"sp{i}" for i in range(clf.num_species())], sensitivity=1.0)
    rate, n = tiny_cfg.sample_rate, tiny_cfg.n_samples
    o = S.Orchestrator()
    o.register("tiny", bn, S.ModelSpec(rate, 3.0, clip_bytes=n * 2))
    errors = []
    wb = S.WindowBatcher(o, R.ResultsQueue(size=1000), max_batch=8, clock=lambda: 9.0, native=native, on_error=lambda *a: errors.append(a))
    for s in ("a", "b", "c"):
        wb.allocate(s, "tiny")
    wb.set_audio_level("a")
    wb.set_audio_level("b", name="mic-b")
    wb.set_processing("a", rate, None, 6.0)                     # the meter sees the frame as given, before the gain
    rng = np.random.default_rng(30)
    written = {"a": [], "b": []}
    for k in range(9):
        for s, a in (("a", 300), ("b", 32767), ("c", 1000)):
            size = 0 if (k, s) == (4, "a") else int(rng.integers(1, n))
            v = rng.integers(-a, a + 1, size).astype("<i2")
            if s == "b" and k % 2 == 0:
                v[-1] = -32768
            raw = v.tobytes()
            wb.write(s, raw)
            if s in written:
                written[s].append(raw)
        if k % 2 == 1:
            wb.tick()
    wb.tick()
    got = wb.take_audio_levels()
    assert not errors and wb.take_audio_levels() == []
    assert {r["source"] for r in got} == {"a", "b"}                              # "c" is never measured
    for s, name in (("a", "a"), ("b", "mic-b")):
        want = _want([(0, raw) for raw in written[s]])
        mine = [r for r in got if r["source"] == s]
        assert [(r["level"], r["clipping"]) for r in mine] == [(w[2], bool(w[3])) for w in want]
        assert all(r["name"] == name and r["timestamp"] == 9.0 for r in mine)
        ref = levelref.Stats()
        for w in want:
            ref.record(w[2], w[3])
        assert wb.audio_level_stats(s) == ref.fields()
    assert any(r["clipping"] for r in got if r["source"] == "b") and any(r["level"] == 0 for r in got if r["source"] == "a")
    assert wb.audio_level_stats("b", reset=True)["count"] == 9 and wb.audio_level_stats("b")["count"] == 0
    with pytest.raises(S.StreamError):
        wb.audio_level_stats("c")
    wb.clear_audio_level("a")
    wb.write("a", np.full(100, 900, "<i2").tobytes())
    wb.tick()
    assert wb.take_audio_levels() == []
    wb.close()
    clf.close()
