"""The capture bank on the device: writes and cuts byte for byte against the restatement (tests/capref.py), the export against the
entries it fuses run one after the other, and WindowBatcher(capture=...) on the tiny model against the test's own copy of the streams."""
import ctypes as C

import numpy as np
import pytest

from birdnet_go_amd import flac, host, spectrogram, wav

import capref

pytestmark = pytest.mark.gpu

CAP, N_SRC = 2048, 3


def _spans(items):
    """[(source, start, length), ...] -> CLIP_SPAN"""
    q = np.zeros(len(items), host.CLIP_SPAN)
    for i, (s, a, n) in enumerate(items):
        q[i] = (a, n, s)
    return q


class Pair:
    """A device bank and the restatement side by side."""

    def __init__(self, max_sources=N_SRC, cap=CAP, rate=48000):
        self.dev = host.CaptureBank(max_sources, 0, rate, capacity_samples=cap)
        self.ref = capref.Bank(max_sources, cap)
        assert self.dev.capacity == self.ref.capacity

    def write(self, frames, bits=16):
        self.dev.write(frames, bits)
        self.ref.write(frames, bits)
        self.same_positions()

    def same_positions(self):
        got, want = self.dev.positions(), self.ref.positions()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (got, want)
        return got

    def read(self, spans):
        assert self.ref.valid(spans)
        got, want = self.dev.read(spans), self.ref.read(spans)
        assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
        return got

    def whole(self):
        """everything every ring holds, as one span per source"""
        wr, old = self.same_positions()
        return self.read(_spans([(s, int(old[s]), int(wr[s] - old[s])) for s in range(len(wr))]))

    def close(self):
        self.dev.close()


def _pcm(rng, n, bits):
    """n samples of `bits` as bytes: noise, with the values that decide the rounding and the clamp planted in front."""
    if bits == 16:
        return rng.integers(-32768, 32768, n).astype("<i2").tobytes()
    if bits == 32:
        v = rng.integers(-2 ** 31, 2 ** 31, n).astype("<i4")
        edge = np.array([0x8000, 0x18000, -0x8000, -0x18000, 0x7FFFFFFF, -0x80000000, 0x7FFF8000, 0x7FFF7FFF], np.int64).astype("<i4")
        v[:min(n, edge.size)] = edge[:n]
        return v.tobytes()
    v = rng.integers(-2 ** 23, 2 ** 23, n).astype(np.int32)
    edge = np.array([0x80, 0x180, 0x280, -0x80, -0x180, 0x7FFFFF, -0x800000, 0x7FFF7F, 0x7FFF80], np.int32)
    v[:min(n, edge.size)] = edge[:n]
    return np.stack([(v >> s) & 0xFF for s in (0, 8, 16)], 1).astype(np.uint8).tobytes()


# ------------------------------------------------------------------------------------------ write and read
@pytest.mark.parametrize("bits", [16, 24, 32])
def test_write_read_round_trip(gpu, bits):
    """Frames of every length class begun at every cell residue mod 8, wrapping frames, several frames of one source in one call and
    a call whose frames of one source total more than the ring; after every call the whole of every ring equals the restatement's."""
    rng = np.random.default_rng(bits)
    p = Pair()
    size = bits // 8
    assert p.dev.capacity == CAP and p.dev.rate == 48000
    residues = set()
    for n in (1, 7, 8, 9, 1023, 2047, 2048, 2049, 5000):
        for lead in (0, 1, 2, 3, 4, 5, 6, 7):                              # the frame begins at another residue every time
            wr = p.same_positions()[0]
            frames = []
            if lead:
                frames.append((1, _pcm(rng, lead, bits)))
            residues.add(int(wr[1] + lead) % 8)
            frames += [(1, _pcm(rng, n, bits)), (0, _pcm(rng, 0, bits)), (2, _pcm(rng, (n * 3) % 700, bits))]
            p.write(frames, bits)
            p.whole()
        if n == 2049:
            assert p.dev.positions()[1][1] > 0                            # source 1 has wrapped
    assert residues == set(range(8))
    # two and three frames of one source in one call; source 2's total more than the ring
    p.write([(0, _pcm(rng, 300, bits)), (2, _pcm(rng, 1500, bits)), (0, _pcm(rng, 9, bits)), (2, _pcm(rng, 1000, bits)), (0, _pcm(rng, 2000, bits)),
             (2, _pcm(rng, 77, bits))], bits)
    p.whole()
    wr, old = p.same_positions()
    assert (wr - old == CAP).all()
    if bits == 16:                                                        # the identity
        x = rng.integers(-32768, 32768, 500).astype("<i2")
        p.write([(1, x.tobytes())])
        assert np.array_equal(p.read(_spans([(1, int(p.dev.positions()[0][1]) - 500, 500)]))[0], x)
    else:                                                                 # ties and saturation reach the ring as the rule has them
        edge = capref.pcm16(_pcm(rng, 9, bits), bits)[:7]
        p.write([(1, _pcm(rng, 9, bits))], bits)
        got = p.read(_spans([(1, int(p.dev.positions()[0][1]) - 9, 7)]))[0]
        assert np.array_equal(got, edge) and 32767 in got.tolist() and -32768 in got.tolist()
    assert size * 8 == bits
    p.close()


def test_reads(gpu):
    rng = np.random.default_rng(3)
    p = Pair()
    p.write([(0, _pcm(rng, 5000, 16)), (1, _pcm(rng, 3000, 16)), (2, _pcm(rng, 1000, 16))])     # 0 and 1 have wrapped, 2 has not
    wr, old = p.same_positions()
    assert old.tolist() == [5000 - CAP, 3000 - CAP, 0]
    # every (source cell mod 8, output offset mod 8) at lengths 1..17 and the whole ring
    for src_res in range(8):
        for out_res in range(8):
            first = int(old[0]) + (src_res - int(old[0])) % 8
            items = ([(1, int(old[1]) + 5, out_res)] if out_res else []) + [(0, first, n) for n in range(1, 18)]
            items.append((0, int(old[0]), CAP))
            items.append((0, first + 8 * 3, 17))
            got = p.read(_spans(items))
            assert len(got) == len(items)
    # spans across the wrap (source 0's cell 0 is position 4096), overlapping spans, a source that has not wrapped yet
    assert old[0] < 4096 < wr[0]
    p.read(_spans([(0, 4096 - 100, 300), (0, 4096 - 50, 300), (0, 4096 - 1, 2), (2, 0, 1000), (2, 999, 1), (1, int(old[1]), CAP), (0, 4095, 1)]))
    # 300 spans in one call, spans of length 0 among them; the same call twice gives the same bytes
    many = []
    for i in range(300):
        s = int(rng.integers(0, 3))
        n = 0 if i % 50 == 7 else int(rng.integers(1, min(600, int(wr[s] - old[s]))))
        many.append((s, int(rng.integers(old[s], wr[s] - n + 1)), n))
    a, b = p.read(_spans(many)), p.dev.read(_spans(many))
    assert len(a) == 294 and all(np.array_equal(x, y) for x, y in zip(a, b))
    p.close()


def test_refusals_and_reset(gpu):
    rng = np.random.default_rng(4)
    p = Pair()
    p.write([(0, _pcm(rng, 5000, 16)), (1, _pcm(rng, 100, 16))])
    wr, old = p.same_positions()

    def refused(call, *args, **kw):
        with pytest.raises(host.HipError) as e:
            call(*args, **kw)
        assert e.value.code == host.E_INVALID
        got = p.dev.positions()
        assert np.array_equal(got[0], wr) and np.array_equal(got[1], old)   # nothing changed

    refused(p.dev.read, _spans([(0, int(old[0]) - 1, 10)]))              # reaches before oldest
    refused(p.dev.read, _spans([(0, int(wr[0]) - 5, 6)]))                # reaches beyond written
    refused(p.dev.read, _spans([(1, 0, 10), (1, 95, 6)]))
    refused(p.dev.read, _spans([(N_SRC, 0, 1)]))                         # a source outside the bank
    refused(p.dev.read, _spans([(-1, 0, 1)]))
    refused(p.dev.read, _spans([(0, int(old[0]), -1)]))
    refused(p.dev.read, _spans([]))                                      # n_spans outside 1..65535
    refused(p.dev.write, [(N_SRC, _pcm(rng, 10, 16))])
    refused(p.dev.write, [(0, _pcm(rng, 10, 16)), (-1, _pcm(rng, 10, 16))])
    refused(p.dev.write, [(0, b"\0" * 8)], 8)                             # depth 8
    lib = host._capture_bank_protos(host.load_library())
    n_neg, src = np.array([-1], np.int64), np.array([0], np.int32)
    ptr = (C.c_void_p * 1)(None)
    assert lib.bnhip_capture_bank_write(p.dev._h, 1, src.ctypes.data, n_neg.ctypes.data, ptr, 16) == host.E_INVALID      # a negative frame length
    assert lib.bnhip_capture_bank_write(None, 0, None, None, None, 16) == host.E_INVALID
    assert lib.bnhip_capture_bank_read_pcm16(p.dev._h, None, 1, None) == host.E_INVALID
    h = C.c_void_p()
    for bad in ((0, 1024, 48000), (65536, 1024, 48000), (1, 0, 48000), (1, 2 ** 31 - 1023, 48000), (1, 1024, 0), (1, 1024, 1 << 20)):
        assert lib.bnhip_capture_bank_create(0, bad[0], bad[1], bad[2], C.byref(h)) == host.E_INVALID and not h.value, bad
    p.same_positions()
    p.read(_spans([(0, int(old[0]), 10), (1, 0, 100)]))                  # a valid call after the refusals
    p.write([(1, _pcm(rng, 10, 16))])
    # reset: positions go to 0 and an old span is refused
    p.dev.reset(0)
    p.ref.reset(0)
    wr, old = p.same_positions()
    assert (wr[0], old[0]) == (0, 0) and wr[1] == 110
    refused(p.dev.read, _spans([(0, 0, 1)]))
    refused(p.dev.reset, N_SRC)
    p.write([(0, _pcm(rng, 33, 16))])
    p.whole()
    p.dev.reset()
    p.ref.reset()
    assert p.same_positions()[0].tolist() == [0, 0, 0]
    small = host.CaptureBank(1, 0, 48000, capacity_samples=1025)          # the capacity is rounded up to 1024 samples
    assert small.capacity == 2048
    small.close()
    p.close()


# ------------------------------------------------------------------------------------------ the export
RATE = 48000


@pytest.fixture(scope="module")
def rings(gpu):
    """A ring of 16 384 samples per source, wrapped, holding tones in noise; the three clips, one across the wrap."""
    rng = np.random.default_rng(9)
    bank = host.CaptureBank(2, 0, RATE, capacity_samples=16384)
    assert bank.capacity == 16384
    t = np.arange(40000) / RATE
    for s in range(2):
        x = (np.clip(0.3 * np.sin(2 * np.pi * (900 + 700 * s) * t) * (1 + np.sin(2 * np.pi * 3 * t)) + rng.normal(0, 0.02, t.size), -1, 1) * 32767)
        bank.write([(s, x.astype("<i2").tobytes())])
    wr, old = bank.positions()
    assert wr.tolist() == [40000, 40000] and old.tolist() == [40000 - 16384] * 2
    # cell 0 is position 32768: the second clip lies across it
    spans = _spans([(0, 24001, 4097), (1, 30000, 6000), (1, 0, 0), (0, 27999, 12001)])
    yield bank, spans
    bank.close()


def _settings(normalize, lpc_order, width):
    return host.ClipSettings(1, 1, 1, False, bool(normalize), seek_interval=RATE // 8, lpc_order=lpc_order, width=width,
                             palette=spectrogram.palette() if width else None)


def _composed(bank, spans, x):
    clips = bank.read(spans)
    if x.normalize:
        loud, fl = host.loudness_flac_ragged(clips, RATE, seek_interval=x.seek_interval, lpc_order=x.lpc_order)
        gained = host.loudness_normalize_ragged(clips, RATE)[1]
    else:
        loud, fl, gained = None, host.flac_encode_ragged(clips, RATE, None, x.seek_interval, lpc_order=x.lpc_order), clips
    png = host.spectrogram_png_ragged(gained, RATE, x.width, spectrogram.palette()) if x.width else None
    return {"clips": clips, "loud": loud, "flac": fl, "png": png}


def _offsets(streams):
    return np.concatenate(([0], np.cumsum([len(s) for s in streams]))).astype(np.uint64)


def _same_export(got, want, n):
    assert got.n_clips == n
    assert got.flac == want["flac"][:n] and np.array_equal(got.flac_offsets[:n + 1], _offsets(want["flac"][:n]))
    assert (got.flac_offsets[n + 1:] == 2 ** 64 - 1).all()
    if want["loud"] is None:
        assert got.loudness is None
    else:
        assert [bytes(r) for r in got.loudness] == [bytes(r) for r in want["loud"][:n]]
    if want["png"] is None:
        assert got.png is None
    else:
        assert got.png == want["png"][:n] and np.array_equal(got.png_offsets[:n + 1], _offsets(want["png"][:n]))


@pytest.mark.parametrize("width", [0, 64])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("lpc_order", [0, 8])
def test_export_against_composed(rings, lpc_order, normalize, width):
    bank, spans = rings
    x = _settings(normalize, lpc_order, width)
    assert not width or (x.width, x.height) == (64, 33)
    want = _composed(bank, spans, x)
    assert [c.size for c in want["clips"]] == [4097, 6000, 12001]
    got = bank.export_raw(spans, x)
    assert np.array_equal(got.spans, spans)                               # the spans as given
    _same_export(got, want, 3)
    assert all(s[:4] == b"fLaC" for s in got.flac) and (not width or all(s[:8] == b"\x89PNG\r\n\x1a\n" for s in got.png))
    if not normalize:                                                     # the streams decode to the ring's own samples
        dec = flac.decode_clips(got.flac)[0]
        assert all(np.array_equal(d, c) for d, c in zip(dec, want["clips"]))
    made = bank.export(spans, x)
    assert [m["flac"] for m in made] == want["flac"] and [int(m["span"]["length"]) for m in made] == [4097, 6000, 12001]


def test_export_capacity_and_refusals(rings):
    bank, spans = rings
    x = _settings(1, 8, 64)
    want = _composed(bank, spans, x)
    two = host.flac_ragged_max_bytes([4097, 6000], x.seek_interval)
    full = host.flac_ragged_max_bytes([4097, 6000, 12001], x.seek_interval)
    _same_export(bank.export_raw(spans, x, flac_cap=full - 1), want, 2)
    _same_export(bank.export_raw(spans, x, flac_cap=two), want, 2)        # room for only two clips
    _same_export(bank.export_raw(spans, x, png_cap=host.png_max_bytes(1, x.width, x.height)), want, 1)
    none = bank.export_raw(spans, x, flac_cap=0)
    assert none.n_clips == 0 and (none.flac_offsets == 2 ** 64 - 1).all() and (none.png_offsets == 2 ** 64 - 1).all()   # no stream written
    wr, old = bank.positions()
    for bad in (_spans([(0, int(old[0]) - 1, 4097)]), _spans([(0, 40000 - 10, 11)]), _spans([(2, 30000, 10)]), _spans([])):
        with pytest.raises(host.HipError) as e:
            bank.export_raw(bad, x)
        assert e.value.code == host.E_INVALID
    with pytest.raises(host.HipError) as e:
        bank.export_raw(spans, host.ClipSettings(1, 1, 1, lpc_order=9))
    assert e.value.code == host.E_INVALID
    got = bank.positions()
    assert np.array_equal(got[0], wr) and np.array_equal(got[1], old)
    _same_export(bank.export_raw(spans, x), want, 3)                      # the bank stays usable


# ------------------------------------------------------------------------------------------ WindowBatcher(capture=...)
def test_window_batcher_capture(gpu, tiny_cfg, tiny_blob):
    """Two sources through WindowBatcher(events=..., capture=...): every clip's FLAC decodes to the slice of the test's own copy of
    the stream at the span the restatement computes from the event, and an event whose clip ends behind what has been written when
    it becomes due is delivered by a later tick, whole."""
    from birdnet_go_amd import results as R, stream as S
    clf = host.HipClassifier(tiny_blob, device=0, max_batch=8)
    nc = clf.num_species()
    labels = [f"sp{i}" for i in range(nc)]
    bn = host.BirdNET(clf, labels, sensitivity=1.0)
    n = tiny_cfg.n_samples
    rate = tiny_cfg.sample_rate
    spec = S.ModelSpec(rate, 3.0, clip_bytes=n * 2)
    overlap, hop = n // 2, n - n // 2
    # every class the model ranks is a hit (thresholds below any output, one class shut out): events open at every window and are
    # due `hold` windows later - the detections are planted by the filter, whatever the audio
    thr = np.full(nc, -1.0, np.float32)
    thr[0] = np.inf
    hold = 2
    flt = host.EventTables(thr, None, 0.0, hold, 1, 0)
    pre, post = hop // 2, 5 * hop                                         # the clip ends 5 hops behind its event's first window: later than it is due
    export = wav.ClipExport(length_seconds=(pre + post) / rate, pre_capture_seconds=pre / rate, normalize=False, lpc_order=8)
    x = export.settings(rate)
    assert (x.pre_samples, x.post_samples) == (pre, post)
    rng = np.random.default_rng(17)
    n_win = 10
    t = np.arange(hop * (n_win + 1)) / rate
    streams = {f"src{i}": (np.clip(0.4 * np.sin(2 * np.pi * (600 + 400 * i) * t) + rng.normal(0, 0.05, t.size), -1, 1) * 32767).astype("<i2") for i in range(2)}
    o = S.Orchestrator()
    o.register("tiny", bn, spec)
    seen = []
    wb = S.WindowBatcher(o, R.ResultsQueue(size=1000), max_batch=8, events=flt, capture=S.CaptureSettings(60 * hop / rate, export, max_sources=4),
                         on_clips=lambda m, clips: seen.extend(clips))
    for s in streams:
        wb.allocate(s, "tiny")
    events, per_tick, waited = [], [], 0
    step = hop // 2 + 13
    for lo in range(0, t.size, step):
        for s, x16 in streams.items():
            wb.write(s, x16[lo:lo + step].tobytes())
        wb.tick()
        events += wb.take_events()
        waited = max(waited, len(wb.capture_waiting.get("tiny", [])))
        per_tick.append(len(seen))
    clips = wb.take_clips()
    assert clips == seen and wb.take_clips() == [] and set(wb.capture_banks) == {"tiny"}
    bank = wb.capture_banks["tiny"]
    assert bank.rate == rate and bank.positions()[0][:2].tolist() == [t.size, t.size]
    assert waited > 0 and len(set(per_tick)) > 2                          # events waited for their audio, and clips came on several ticks
    # what the restatement expects of the events, on the final clocks: nothing has left the rings, every clip is whole
    ev = np.zeros(len(events), host.EVENT)
    for i, e in enumerate(events):
        ev[i] = (int(e["source"][3:]), e["class_index"], e["first_window"], e["last_window"], e["best_window"], e["count"], e["confidence"], e["status"])
    wr, old = bank.positions()
    spans, status = capref.spans(ev, wr, old, hop, pre, post, x.max_samples, False, np.full(4, -overlap, np.int64))
    done = [i for i in range(len(events)) if status[i] in (capref.OK, capref.CLAMPED)]
    assert len(done) >= 8 and capref.CLAMPED in status.tolist() and capref.NOT_YET in status.tolist()
    key = lambda source, c, fw: (source, int(c), int(fw))
    got = {key(c["source"], c["class_index"], c["first_window"]): c for c in clips}
    assert len(got) == len(clips) == len(done)                            # the events still waiting have no clip, cut short or otherwise
    decoded = flac.decode_clips([c["flac"] for c in clips])[0]
    for c, d in zip(clips, decoded):
        assert np.array_equal(d, streams[c["source"]][c["start"]:c["start"] + c["length"]]) and c["png"] is None and c["loudness"] is None
    for i in done:
        c = got[key(events[i]["source"], events[i]["class_index"], events[i]["first_window"])]
        assert (c["start"], c["length"], c["status"]) == (int(spans[i]["start"]), int(spans[i]["length"]), int(status[i])), (c, spans[i])
        assert c["length"] == (pre + post if status[i] == capref.OK else pre + post + (events[i]["first_window"] * hop - overlap - pre))
    # remove(source) resets that source's ring
    wb.remove("src1")
    assert bank.positions()[0][:2].tolist() == [t.size, 0]
    wb.close()
    assert not wb.capture_banks
    clf.close()
