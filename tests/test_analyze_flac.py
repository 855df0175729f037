"""File analysis of FLAC recordings in one device call (bnhip_analyze_flac_windows / _topk / bnhip_analyze_flac / _events,
wav.analyze_files on FLAC files).

The criterion is bit identity - np.array_equal - with the bnhip_analyze_channels_* calls on the PCM that tests/flacwidedec.py, the
decoder restatement, makes of the same streams: the decoder writes the bytes the channels call's copies would have brought, and
everything behind them is the channels call's own code, so no tolerance appears.  The model and the window geometry are those of
tests/test_analyze_channels.py.  Three recordings: stereo 16-bit at the model's rate, stereo 24-bit at 32 kHz, mono 16-bit of 2.4
windows; long spans are VERBATIM and FIXED subframes (the muxer stays fast), one frame of each recording is LPC."""
import struct

import numpy as np
import pytest

import flacwidecases as FK
import flacwidedec as D
import flacwidemux as M
from birdnet_go_amd import flac, host, wav

from test_analyze import _fft_tiny_blob
from test_analyze_mixed_ref import CLIP, HOP, K, MIN_TAIL, MODEL_RATE

pytestmark = pytest.mark.gpu

SHAPES = ((MODEL_RATE, 16, 30011, 2), (32000, 24, 20001, 2), (MODEL_RATE, 16, int(2.4 * CLIP), 1))      # rate, bits, frames, channels
BS = 4096


def _recording(rate, bits, n, channels, seed):
    rng = np.random.default_rng(seed)
    full = 1 << (bits - 1)
    t = np.arange(n)[:, None]
    c = np.arange(channels)[None, :]
    x = (0.1 + 0.25 * c) * np.sin(2 * np.pi * (400.0 + 300.0 * c) * t / rate) + 0.02 * rng.standard_normal((n, channels))
    x = np.clip(np.round(x * full), -full, full - 1).astype(np.int64)
    assign = (0,) if channels == 1 else (8, 10, 1, 9)
    frames = []
    for j in range(-(-n // BS)):
        sub = FK.lpc(8) if j == 1 else dict(kind="VERBATIM") if j % 2 else dict(kind="FIXED", order=2)
        frames.append(dict(assign=assign[j % len(assign)], sub=sub))
    return M.stream(x, bits, BS, rate, frames), x


@pytest.fixture(scope="module")
def material():
    made = [_recording(*shape, seed=50 + i) for i, shape in enumerate(SHAPES)]
    streams = [s for s, _ in made]
    pcm = []
    for (s, x), (_, bits, _, _) in zip(made, SHAPES):
        y = D.decode(s)[0]
        assert np.array_equal(y, x)
        pcm.append(D.pcm_bytes(y, bits))
    return streams, pcm


@pytest.fixture(scope="module")
def engine(gpu):
    c = host.HipClassifier(_fft_tiny_blob(), max_batch=32, autotune=False, lanes=2)
    yield c
    c.close()


def _select(choice):
    """One choice for the burst; the mono recording has no channel 1."""
    return [choice, choice, 0 if choice == 1 else choice]


def _recs(select, shapes=SHAPES):
    return host.channel_recordings([s[2] for s in shapes], [s[0] for s in shapes], [s[1] for s in shapes], [s[3] for s in shapes], select)


def _ok(results, n):
    assert [(int(r["status"]), int(r["fail_offset"])) for r in results] == [(host.FLAC_OK, 0)] * n


def test_windows_equal_the_channels_table(material):
    streams, _ = material
    got = host.analyze_flac_windows(streams, MODEL_RATE, CLIP, HOP, MIN_TAIL)
    want = host.analyze_channels_windows(_recs(0), MODEL_RATE, CLIP, HOP, MIN_TAIL)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and int(got[0][-1]) > 8


@pytest.mark.parametrize("choice", [0, 1, "mix", "auto"])
def test_topk_rows_and_events_equal_the_channels_calls_on_the_restatement_pcm(engine, material, choice):
    streams, pcm = material
    c, sel, raw = engine, _select(choice), b"".join(pcm)
    conf, idx, first, chosen, results = c.analyze_flac_topk(streams, sel, MODEL_RATE, HOP, MIN_TAIL, k=K)
    wconf, widx, wfirst, wchosen = c.analyze_channels_pcm_topk(raw, _recs(sel), MODEL_RATE, HOP, MIN_TAIL, k=K)
    _ok(results, 3)
    assert np.isfinite(conf).all() and np.array_equal(conf, wconf) and np.array_equal(idx, widx)
    assert np.array_equal(first, wfirst) and np.array_equal(chosen, wchosen)
    assert [int(r["frames"]) for r in results] == [-(-s[2] // BS) for s in SHAPES]
    threshold = float(np.median(conf))
    rows, total, chosen, results = c.analyze_flac(streams, sel, MODEL_RATE, HOP, MIN_TAIL, k=K, threshold=threshold)
    wrows, wtotal, wchosen = c.analyze_channels_pcm(raw, _recs(sel), MODEL_RATE, HOP, MIN_TAIL, k=K, threshold=threshold)
    _ok(results, 3)
    assert total == wtotal and 0 < total < conf.size and np.array_equal(rows, wrows) and np.array_equal(chosen, wchosen)
    flt = wav.EventFilter(default_threshold=threshold).tables(c.num_species(), MODEL_RATE, HOP)
    ev, chosen, results = c.analyze_flac_events(streams, sel, MODEL_RATE, HOP, flt, MIN_TAIL, k=K)
    wev, wchosen = c.analyze_channels_pcm_events(raw, _recs(sel), MODEL_RATE, HOP, flt, MIN_TAIL, k=K)
    _ok(results, 3)
    assert np.array_equal(ev, wev) and np.array_equal(chosen, wchosen)


def test_a_plain_burst_takes_the_fast_path_to_the_same_answers(engine, material):
    streams, pcm = material
    got = engine.analyze_flac_topk([streams[2], streams[2]], "mix", MODEL_RATE, HOP, MIN_TAIL, k=K)
    want = engine.analyze_pcm_topk(pcm[2] * 2, 16, [SHAPES[2][2]] * 2, HOP, MIN_TAIL, k=K)
    _ok(got[4], 2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def test_a_plain_burst_of_24_bit_mono_sends_the_wide_restore_into_the_slots(engine):
    """Mono 24-bit at the model's rate is plain too: the wide restore writes packed 3-byte samples straight into the slot block."""
    lengths = (int(1.3 * CLIP) + 1, int(2.1 * CLIP))                 # (an odd count of 3-byte samples in front of the second slot)
    made = [_recording(MODEL_RATE, 24, n, 1, seed=70 + i) for i, n in enumerate(lengths)]
    pcm = b"".join(D.pcm_bytes(D.decode(s)[0], 24) for s, _ in made)
    got = engine.analyze_flac_topk([s for s, _ in made], 0, MODEL_RATE, HOP, MIN_TAIL, k=K)
    want = engine.analyze_pcm_topk(pcm, 24, list(lengths), HOP, MIN_TAIL, k=K)
    _ok(got[4], 2)
    assert np.isfinite(got[0]).all() and got[0].shape[0] >= 3
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def test_a_damaged_recording_does_not_fail_the_call(engine, material):
    streams, pcm = material
    starts = [f["start"] for f in D.decode(streams[1])[1]["frames"]]
    bad = bytearray(streams[1])
    bad[starts[2] + 100] ^= 0x04
    burst = [streams[0], bytes(bad), streams[2]]
    decoded, dres = flac.decode_recordings(burst, as_bytes=True)
    assert (dres[1].status, dres[1].frames, dres[1].fail_offset) == (host.FLAC_CORRUPT, 2, starts[2])
    pitch = 6
    assert decoded[1][:2 * BS * pitch] == pcm[1][:2 * BS * pitch] and not any(decoded[1][2 * BS * pitch:]) and decoded[0] == pcm[0]
    conf, idx, first, chosen, results = engine.analyze_flac_topk(burst, "mix", MODEL_RATE, HOP, MIN_TAIL, k=K)
    assert [int(r["status"]) for r in results] == [host.FLAC_OK, host.FLAC_CORRUPT, host.FLAC_OK]
    assert (int(results[1]["frames"]), int(results[1]["fail_offset"])) == (2, starts[2])
    want = engine.analyze_channels_pcm_topk(b"".join(decoded), _recs("mix"), MODEL_RATE, HOP, MIN_TAIL, k=K)
    assert np.array_equal(conf, want[0]) and np.array_equal(idx, want[1]) and np.array_equal(chosen, want[3])
    whole = engine.analyze_flac_topk(streams, "mix", MODEL_RATE, HOP, MIN_TAIL, k=K)
    a, b, c = int(first[1]), int(first[2]), int(first[3])
    assert np.array_equal(conf[:a], whole[0][:a]) and np.array_equal(conf[b:c], whole[0][b:c]) and not np.array_equal(conf[a:b], whole[0][a:b])


def test_each_refusal_has_its_own_text(engine, material):
    streams, _ = material

    def refused(burst, select, *, hop=HOP):
        with pytest.raises(host.HipError) as e:
            engine.analyze_flac_topk(burst, select, MODEL_RATE, hop, MIN_TAIL, k=K)
        assert e.value.code == host.E_INVALID
        return str(e.value)

    texts = [refused([streams[0], b"RIFF" + streams[1][4:]], 0), refused([streams[0], streams[1][:30]], 0),
             refused([streams[0], FK.above_cap()], 0), refused([streams[0], FK.cases()["kinds_mid_side_16"][0][:41]], 0),
             refused(streams, [0, 2, 0]), refused(streams, [0, 0, 1]), refused(streams, 0, hop=CLIP + 1), refused(streams, 0, hop=0)]
    assert "recording 1: not a FLAC stream" in texts[0] and "recording 1: not a FLAC stream" in texts[1]
    assert "recording 1: a FLAC stream of 2 channels, 24 bits, block size 8193 is not decoded" in texts[2]
    assert "recording 1: not a FLAC stream" in texts[3]
    assert "recording 1" in texts[4] and "select" in texts[4] and "recording 2" in texts[5] and "select" in texts[5]
    assert "hop" in texts[6] and "hop" in texts[7]
    assert len({texts[0], texts[2], texts[4], texts[5], texts[6]}) == 5
    # the handle stays usable
    assert engine.analyze_flac_topk(streams, 0, MODEL_RATE, HOP, MIN_TAIL, k=K)[0].shape[1] == K


def _wav_bytes(raw, rate, bits, channels):
    return (b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " +
            struct.pack("<IHHIIHH", 16, 1, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits) + b"data" + struct.pack("<I", len(raw)) + raw)


def test_analyze_files_on_flac_files_equals_the_same_files_as_wav(engine, material, tmp_path):
    streams, pcm = material
    wavs = [_wav_bytes(p, s[0], s[1], s[3]) for p, s in zip(pcm, SHAPES)]
    path = tmp_path / "second.flac"
    path.write_bytes(streams[1])
    files = [streams[0], str(path), streams[2]]
    for kw in (dict(channels="auto"), dict(channels="mix", events=wav.EventFilter(default_threshold=0.05))):
        got = wav.analyze_files(files, engine, model_rate=MODEL_RATE, top_k=K, return_chosen=True, **kw)
        want = wav.analyze_files(wavs, engine, model_rate=MODEL_RATE, top_k=K, return_chosen=True, **kw)
        assert got == want and len(got[0]) == 3
        assert "events" in kw or sum(len(r) for r in got[0]) > 0
    with pytest.raises(wav.WavError, match="FLAC recordings only"):
        wav.analyze_files([streams[0], wavs[1]], engine, model_rate=MODEL_RATE, channels=0)
    with pytest.raises(ValueError, match="channels set"):
        wav.analyze_files(files, engine, model_rate=MODEL_RATE)
    for kw in (dict(export=wav.ClipExport()), dict(extend=wav.ExtendedCapture(max_seconds=60.0)), dict(guards=wav.EventGuards(0.5))):
        with pytest.raises(ValueError, match="not offered for FLAC"):
            wav.analyze_files(files, engine, model_rate=MODEL_RATE, channels=0, events=wav.EventFilter(), **kw)
    bad = bytearray(streams[1])
    bad[len(bad) // 2] ^= 0x20
    with pytest.raises(wav.WavError, match=r"<\d+ bytes>: damaged FLAC stream: frame \d+ at byte \d+"):
        wav.analyze_files([streams[0], bytes(bad)], engine, model_rate=MODEL_RATE, channels="mix")
