"""Detection clips from analysed recordings: the cut alone (bnhip_recording_clips_pcm16) against numpy, and the fused
bnhip_analyze_channels_pcm_clips against the composition of the entries it fuses - the events call, the span rule (tests/clipref.py),
the cut, bnhip_loudness_flac_ragged_pcm16 and bnhip_spectrogram_png_ragged_pcm16 - with the tiny FFT model and the five-recording
burst of tests/test_analyze.py.

Every comparison is np.array_equal or a bytes comparison: every stage is pinned bit for bit by its own tests, and the cut is a
conversion with one stated rounding."""
import ctypes as C

import numpy as np
import pytest

from birdnet_go_amd import host, spectrogram, wav

import chanref
import clipref
import evref
import flacdec
import flaclpcdec
from test_analyze import CLIP, HOP, K, LENGTHS, MIN_TAIL, _bytes, _fft_tiny_blob, _recordings, _write_wav16
from test_analyze_events import _between, _flt

pytestmark = pytest.mark.gpu

RATE, TILE, WIDTH = 48000, 2048, 128


def _span_table(items):
    t = np.zeros(len(items), host.CLIP_SPAN)
    for i, (r, start, length) in enumerate(items):
        t[i] = (start, length, r)
    return t


# ------------------------------------------------------------------------------------------ the cut alone
# (recording, start, length): the lengths around a lane's line of 8 and around the kernel's tile, at odd and even starts - the
# packed output starts each clip wherever the one before ended, so the lines' heads and tails come in every width; whole recordings
# (the 7-sample one, and the long one: 153 tiles); two overlapping spans; a span of length 0 between two others
CUT_SPANS = [(0, 0, 1), (0, 1, 2), (0, 3, 7), (0, 10, 8), (0, 21, 9), (4, 1001, TILE - 1), (4, 4000, TILE), (4, 7, TILE + 1), (1, 0, 7),
             (2, 0, CLIP), (3, 5000, 3000), (3, 6001, 3000), (0, 100, 0), (2, CLIP - 1, 1), (4, 0, LENGTHS[4]), (0, 5 * CLIP - 5, 8)]


def _float_specials(x):
    """float32 material with values beyond +-1, exact ties, a NaN and infinities in reach of the spans above."""
    x = x.copy()
    x[0:12] = np.array([1.5, -1.5, 0.5, 1.5, 2.5, -0.5, 32766.5, 32767.5, -32768.5, np.nan, np.inf, -np.inf], np.float32) / np.float32(32768.0)
    x[0], x[1] = np.float32(1.5), np.float32(-1.5)
    return x


@pytest.mark.parametrize("bits", [16, 24, 32, 0])
def test_cut_alone(gpu, bits):
    recs = _recordings(LENGTHS)
    raws = [_bytes(x, bits) for x in recs]
    if bits == 0:
        raws = [_float_specials(np.frombuffer(r, "<f4")).tobytes() if i in (0, 4) else r for i, r in enumerate(raws)]
    table = host.channel_recordings(LENGTHS, RATE, bits, 1, 0)
    spans = _span_table(CUT_SPANS)
    want = clipref.cut([clipref.as_float32(r, bits) for r in raws], spans)
    got = host.recording_clips(b"".join(raws), table, RATE, spans)
    assert len(got) == len(want) == len(CUT_SPANS) - 1
    for g, w, s in zip(got, want, [s for s in CUT_SPANS if s[2]]):
        assert g.dtype == np.int16 and np.array_equal(g, w), s
    if bits == 0:
        assert np.isnan(np.frombuffer(raws[0], "<f4")[9]) and got[0][0] == 32767 and got[1][0] == -32768      # (the specials are inside spans)
    else:
        # every depth carries the 16-bit samples: the clip is the source itself
        for g, (r, start, length) in zip(got, [s for s in CUT_SPANS if s[2]]):
            assert g.tobytes() == recs[r][start:start + length].astype("<i2").tobytes()


def test_cut_resampled_and_mixed(gpu):
    """A 44.1 kHz mono recording and a 32 kHz stereo recording read as its mix: the clips are rint of what bnhip_resample_f32 gives
    over the float32 recording of chanref.mix."""
    a, left, right = _recordings([30011, 20005, 20005], seed=41)
    frames = np.stack([left, (right // 3).astype(np.int16)], axis=1).astype(np.int64)
    raw = _bytes(a, 16) + chanref.pack(frames, 16)
    table = host.channel_recordings([a.size, left.size], [44100, 32000], 16, [1, 2], [0, "mix"])
    n_out = host.analyze_channels_windows(table, RATE, CLIP, HOP, MIN_TAIL)[1]
    f0 = host.Resampler(44100, RATE).resample_f32(chanref.to_float(a.astype(np.int64), 16))
    f1 = host.Resampler(32000, RATE).resample_f32(chanref.mix(frames, 16))
    assert [f0.size, f1.size] == n_out.tolist()
    spans = _span_table([(0, 0, int(n_out[0])), (1, 0, int(n_out[1])), (0, 4097, TILE + 3), (1, 12345, 1), (1, int(n_out[1]) - 9, 9)])
    want = clipref.cut([f0, f1], spans)
    got = host.recording_clips(raw, table, RATE, spans)
    assert len(got) == 5 and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert np.abs(got[0].astype(np.int64)).max() > 1000 and np.abs(got[1].astype(np.int64)).max() > 1000


def test_cut_refusals(gpu):
    recs = _recordings(LENGTHS[:2])
    raw, table = _bytes(np.concatenate(recs), 16), host.channel_recordings(LENGTHS[:2], RATE, 16, 1, 0)
    for bad in ([(2, 0, 1)], [(0, -1, 2)], [(1, 0, 8)], [(0, LENGTHS[0], 1)], [(0, 0, -1)], []):
        with pytest.raises(host.HipError) as ei:
            host.recording_clips(raw, table, RATE, _span_table(bad))
        assert ei.value.code == host.E_INVALID, bad
    assert host.recording_clips(raw, table, RATE, _span_table([(0, 5, 0)])) == []
    assert np.array_equal(host.recording_clips(raw, table, RATE, _span_table([(1, 0, 7)]))[0], recs[1])


# ------------------------------------------------------------------------------------------ the fused entry
@pytest.fixture(scope="module")
def clf(gpu):
    c = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False)
    yield c
    c.close()


@pytest.fixture(scope="module")
def burst(clf):
    recs = _recordings(LENGTHS)
    raw = _bytes(np.concatenate(recs), 16)
    table = host.channel_recordings(LENGTHS, RATE, 16, 1, 0)
    rows, _, _ = clf.analyze_channels_pcm(raw, table, RATE, HOP, MIN_TAIL, k=K, threshold=0.0)
    return {"recs": recs, "raw": raw, "table": table, "rows": rows}


def _settings(extended=False, normalize=True, lpc_order=0, width=WIDTH, rate_out=0, seek_interval=0):
    return host.ClipSettings(5000, 15001, 40000 if extended else 2 ** 31 - 1, extended, normalize, seek_interval=seek_interval, lpc_order=lpc_order,
                             width=width, rate_out=rate_out, palette=spectrogram.palette() if width else None)


def _spans_of(ev, x):
    return clipref.spans(ev, LENGTHS, HOP, x.pre_samples, x.post_samples, x.max_samples, x.extended)


def _pick(rows, n_classes, x):
    """A filter (no veto, kept events only) under which the RESTATEMENT gives between 3 and 40 clips of at least 2 distinct lengths:
    a property of the inputs, searched without the code under test."""
    for q in (0.5, 0.65, 0.35, 0.8, 0.2):
        thr = np.full(n_classes, np.inf, np.float32)
        for c in np.unique(rows["class_index"]):
            thr[c] = _between(rows["confidence"][rows["class_index"] == c], q)
        for hold in (3, 5, 2):
            for min_count in (2, 1, 3):
                f = _flt(thr, hold=hold, min_count=min_count)
                lens = _spans_of(evref.events(rows, f), x)["length"]
                if 3 <= lens.size <= 40 and np.unique(lens).size >= 2:
                    return f
    raise AssertionError("the rows give no filter with three clips of two lengths")


def _composed(clf, b, f, x):
    """The entries the fused call fuses, one after the other, every clip crossing to the host and back."""
    ev, chosen = clf.analyze_channels_pcm_events(b["raw"], b["table"], RATE, HOP, f, MIN_TAIL, k=K)
    spans = _spans_of(ev, x)
    clips = host.recording_clips(b["raw"], b["table"], RATE, spans)
    if x.normalize:
        kw = dict(target_lufs=x.target_lufs, true_peak_dbtp=x.true_peak_dbtp, max_gain_db=x.max_gain_db, gate_fallback=x.gate_fallback)
        loud, flac = host.loudness_flac_ragged(clips, RATE, seek_interval=x.seek_interval, lpc_order=x.lpc_order, **kw)
        gained = host.loudness_normalize_ragged(clips, RATE, **kw)[1]
    else:
        loud, flac, gained = None, host.flac_encode_ragged(clips, RATE, None, x.seek_interval, lpc_order=x.lpc_order), clips
    png = host.spectrogram_png_ragged(gained, RATE, x.width, spectrogram.palette(), rate_out=x.rate_out) if x.width else None
    return {"events": ev, "spans": spans, "clips": clips, "gained": gained, "loud": loud, "flac": flac, "png": png}


def _offsets(streams):
    return np.concatenate(([0], np.cumsum([len(s) for s in streams]))).astype(np.uint64)


def _same_export(got, want, n=None):
    n = len(want["flac"]) if n is None else n
    assert got.n_clips == n
    assert got.flac == want["flac"][:n] and np.array_equal(got.flac_offsets[:n + 1], _offsets(want["flac"][:n]))
    if want["loud"] is None:
        assert got.loudness is None
    else:
        assert [bytes(r) for r in got.loudness] == [bytes(r) for r in want["loud"][:n]]
    if want["png"] is None:
        assert got.png is None
    else:
        assert got.png == want["png"][:n] and np.array_equal(got.png_offsets[:n + 1], _offsets(want["png"][:n]))


@pytest.mark.parametrize("normalize,lpc_order,extended,rate_out", [(1, 0, 0, 0), (0, 8, 1, 24000), (1, 8, 1, 24000), (0, 0, 0, 0)])
def test_fused_against_composed(clf, burst, normalize, lpc_order, extended, rate_out):
    x = _settings(bool(extended), bool(normalize), lpc_order, rate_out=rate_out, seek_interval=RATE // 4)
    f = _pick(burst["rows"], clf.num_species(), x)
    want = _composed(clf, burst, f, x)
    lens = [c.size for c in want["clips"]]
    assert len(lens) >= 3 and len(set(lens)) >= 2                         # the comparison cannot pass empty
    got = clf.analyze_channels_pcm_clips(burst["raw"], burst["table"], RATE, HOP, f, x, MIN_TAIL, k=K)
    assert got.n_events == want["events"].size and np.array_equal(got.events, want["events"])
    assert np.array_equal(got.spans, want["spans"]) and got.chosen.tolist() == [0] * len(LENGTHS)
    _same_export(got, want)
    assert all(s[:4] == b"fLaC" for s in got.flac) and all(s[:8] == b"\x89PNG\r\n\x1a\n" for s in got.png)
    dec = flaclpcdec if lpc_order else flacdec                            # (tests/flacdec.py reads the streams without LPC subframes)
    for s, g in zip(got.flac, want["gained"]):                            # the streams decode to the gained clips
        assert np.array_equal(dec.decode(s)[0], g.astype(np.int64))


def test_fused_resampled_stereo(clf):
    """Off the fast path: a 32 kHz stereo recording, the channel left to the device, no images."""
    left, right = _recordings([6 * CLIP + 3, 6 * CLIP + 3], seed=31)
    frames = np.stack([left, (right // 64).astype(np.int16)], axis=1).reshape(-1)
    b = {"raw": _bytes(frames, 16), "table": host.channel_recordings([left.size], 32000, 16, 2, "auto")}
    rows, _, chosen = clf.analyze_channels_pcm(b["raw"], b["table"], RATE, HOP, MIN_TAIL, k=K, threshold=0.0)
    x = _settings(width=0, lpc_order=4)
    n_out = host.analyze_channels_windows(b["table"], RATE, CLIP, HOP, MIN_TAIL)[1]
    thr = np.full(clf.num_species(), np.inf, np.float32)
    for c in np.unique(rows["class_index"]):
        thr[c] = _between(rows["confidence"][rows["class_index"] == c], 0.5)
    f = _flt(thr, hold=3, min_count=1)
    ev, _ = clf.analyze_channels_pcm_events(b["raw"], b["table"], RATE, HOP, f, MIN_TAIL, k=K)
    spans = clipref.spans(ev, n_out, HOP, x.pre_samples, x.post_samples, x.max_samples, x.extended)
    clips = host.recording_clips(b["raw"], b["table"], RATE, spans)
    assert len(clips) >= 1
    loud, flac = host.loudness_flac_ragged(clips, RATE, lpc_order=4)
    got = clf.analyze_channels_pcm_clips(b["raw"], b["table"], RATE, HOP, f, x, MIN_TAIL, k=K)
    assert np.array_equal(got.events, ev) and np.array_equal(got.spans, spans) and got.chosen.tolist() == chosen.tolist() == [0]
    _same_export(got, {"flac": flac, "loud": loud, "png": None})


def test_capacity(clf, burst):
    x = _settings()
    f = _pick(burst["rows"], clf.num_species(), x)
    want = _composed(clf, burst, f, x)
    lens = [c.size for c in want["clips"]]
    n = len(lens)
    full = host.flac_ragged_max_bytes(lens, 0)
    kw = dict(min_tail=MIN_TAIL, k=K, png_cap=host.png_max_bytes(n, x.width, x.height))
    _same_export(clf.analyze_channels_pcm_clips(burst["raw"], burst["table"], RATE, HOP, f, x, flac_cap=full, **kw), want, n)
    short = clf.analyze_channels_pcm_clips(burst["raw"], burst["table"], RATE, HOP, f, x, flac_cap=full - 1, **kw)
    assert clipref.capacity(want["spans"], full - 1, 0, kw["png_cap"], x.width, x.height) == n - 1
    _same_export(short, want, n - 1)                                      # one clip less, the first clips' bytes unchanged
    assert short.n_events == want["events"].size and np.array_equal(short.spans, want["spans"])
    assert short.flac_offsets[n] == 2 ** 64 - 1
    kw["png_cap"] = host.png_max_bytes(2, x.width, x.height)              # the images' room decides
    _same_export(clf.analyze_channels_pcm_clips(burst["raw"], burst["table"], RATE, HOP, f, x, flac_cap=full, **kw), want, 2)
    one = clf.analyze_channels_pcm_clips(burst["raw"], burst["table"], RATE, HOP, f, x, MIN_TAIL, k=K, event_cap=1)
    assert one.n_events == want["events"].size and np.array_equal(one.events, want["events"][:1])
    _same_export(one, want, 1)
    none = clf.analyze_channels_pcm_clips(burst["raw"], burst["table"], RATE, HOP, _flt(np.full(clf.num_species(), np.inf, np.float32)), x,
                                          MIN_TAIL, k=K)
    assert none.n_clips == 0 and none.n_events == 0 and none.events.size == 0
    assert (none.flac_offsets == 2 ** 64 - 1).all() and (none.png_offsets == 2 ** 64 - 1).all()


def test_refusals_leave_the_handle_usable(clf, burst):
    x = _settings()
    f = _pick(burst["rows"], clf.num_species(), x)
    before, _ = clf.analyze_channels_pcm_events(burst["raw"], burst["table"], RATE, HOP, f, MIN_TAIL, k=K)
    dropped = host.EventTables(f.class_threshold, None, 0.0, f.hold_windows, f.min_count, host.EVENTS_KEEP_DROPPED)
    for flt, xs in [(dropped, x), (f, host.ClipSettings(-1, 100, 100)), (f, host.ClipSettings(0, 0, 100)), (f, host.ClipSettings(0, 100, 0)),
                    (f, _settings(lpc_order=9))]:
        with pytest.raises(host.HipError) as ei:
            clf.analyze_channels_pcm_clips(burst["raw"], burst["table"], RATE, HOP, flt, xs, MIN_TAIL, k=K)
        assert ei.value.code == host.E_INVALID
    # NULL outputs, through the C ABI itself
    lib = host._analyze_clips_protos(host.load_library())
    raw = np.frombuffer(burst["raw"], np.uint8)
    fs, xs = f._struct(clf.num_species()), x._struct()
    ev, spans, off = np.zeros(8, host.EVENT), np.zeros(8, host.CLIP_SPAN), np.zeros(9, np.uint64)
    loud, buf = (host.Loudness * 8)(), np.zeros(1 << 20, np.uint8)
    args = dict(events=ev.ctypes.data, event_cap=8, n_events=0, spans=spans.ctypes.data, loudness=C.addressof(loud), flac=buf.ctypes.data,
                flac_cap=buf.size, flac_offsets=off.ctypes.data, png=buf.ctypes.data, png_cap=buf.size, png_offsets=off.ctypes.data, n_clips=0)
    for null in ("events", "spans", "loudness", "flac", "flac_offsets", "png", "png_offsets", None):
        o = host._ClipsOutStruct(**{k: (None if k == null else v) for k, v in args.items()})
        rc = lib.bnhip_analyze_channels_pcm_clips(clf._h, raw.ctypes.data, burst["table"].ctypes.data, burst["table"].size, RATE, HOP, MIN_TAIL, 0,
                                                  1.0, K, C.addressof(fs), None, C.addressof(xs), C.addressof(o) if null is not None else None)
        assert rc == host.E_INVALID and o.n_events == 0 and not ev.tobytes().strip(b"\0"), null
    after, _ = clf.analyze_channels_pcm_events(burst["raw"], burst["table"], RATE, HOP, f, MIN_TAIL, k=K)
    assert after.size and after.tobytes() == before.tobytes()


def test_analyze_files_export(clf, burst, tmp_path):
    """wav.analyze_files(events=..., export=...) on 16-bit WAV files: the tuples without export, each followed by its clip's span,
    FLAC bytes, loudness record and PNG bytes - those of the composition."""
    paths = []
    for i, rec in enumerate(burst["recs"]):
        paths.append(str(tmp_path / f"r{i}.wav"))
        _write_wav16(paths[-1], rec)
    clip_seconds, overlap = CLIP / RATE, (CLIP - HOP) / RATE
    clip_len, hop, min_tail = wav._framing(RATE, clip_seconds, overlap, 1.0)
    assert (clip_len, hop) == (CLIP, HOP)
    rows, _, _ = clf.analyze_channels_pcm(burst["raw"], burst["table"], RATE, HOP, min_tail, k=K, threshold=0.0)
    export = wav.ClipExport(length_seconds=20001 / RATE, pre_capture_seconds=5000 / RATE, lpc_order=8, image=(WIDTH, 65), palette=spectrogram.palette(),
                            rate_out=24000)
    x = export.settings(RATE)
    assert (x.pre_samples, x.post_samples, x.height) == (5000, 15001, host.spectrogram_size(WIDTH)[0])
    f = _pick(rows, clf.num_species(), x)
    finite = np.isfinite(f.class_threshold)
    flt = wav.EventFilter(default_threshold=np.inf, thresholds={int(c): float(f.class_threshold[c]) for c in np.flatnonzero(finite)},
                          hold_seconds=f.hold_windows * HOP / RATE, min_count=f.min_count)
    kw = dict(overlap_seconds=overlap, top_k=K, model_rate=RATE, events=flt)
    plain = wav.analyze_files(paths, clf, **kw)
    ev, _ = clf.analyze_channels_pcm_events(burst["raw"], burst["table"], RATE, HOP, flt.tables(clf.num_species(), RATE, HOP, overlap), min_tail, k=K)
    spans = _spans_of(ev, x)
    clips = host.recording_clips(burst["raw"], burst["table"], RATE, spans)
    loud, flac = host.loudness_flac_ragged(clips, RATE, lpc_order=8)
    png = host.spectrogram_png_ragged(host.loudness_normalize_ragged(clips, RATE)[1], RATE, WIDTH, spectrogram.palette(), rate_out=24000)
    got = wav.analyze_files(paths, clf, export=export, **kw)
    assert [[t[:5] for t in per] for per in got] == plain and sum(len(per) for per in got) == ev.size >= 3
    flat = [t for per in got for t in per]                                # events are ordered by recording first: the clips' order
    assert [t[5:7] for t in flat] == [(int(s["start"]), int(s["length"])) for s in spans]
    assert [t[7] for t in flat] == flac and [bytes(t[8]) for t in flat] == [bytes(r) for r in loud] and [t[9] for t in flat] == png
    few = wav.analyze_files(paths, clf, export=wav.ClipExport(length_seconds=20001 / RATE, pre_capture_seconds=5000 / RATE, lpc_order=8, max_clips=2), **kw)
    flat = [t for per in few for t in per]
    assert [t[7] for t in flat] == flac[:2] + [None] * (len(flac) - 2) and all(t[9] is None for t in flat)
