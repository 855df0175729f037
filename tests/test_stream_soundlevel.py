"""WindowBatcher with a source's sound level monitor (set_sound_level): the 1/3-octave monitor (soundlevel.Processor behind a
SoundLevelConsumer route, internal/analysis/audio_pipeline_service.go:685-740) sees each frame of the source at the source
rate, after set_processing's EQ and gain.  take_sound_levels() equals tests/slref.py run on the tests/eqref.py-processed
frames; the model windows stay those of a batcher without the monitor; native and Python rings agree."""
import numpy as np
import pytest

import eqref
import slref
from birdnet_go_amd import host
from birdnet_go_amd import results as R
from birdnet_go_amd import stream as S

SPEC48 = S.ModelSpec(48000, 3.0, clip_bytes=9600)         # 100 ms windows, 50 % overlap
SPEC32 = S.ModelSpec(32000, 5.0, clip_bytes=6400)
GAIN_DB = 6.0
SOURCES = {"a48": 48000, "b32": 32000}
INTERVAL = {"a48": 1, "b32": 2}


class _Fake:
    def predict_batch(self, flat, n):
        x = np.asarray(flat, np.float32).reshape(n, -1)
        return [[("sp", float(np.float32(0.5) + x[i, 0]))] for i in range(n)]

    def close(self):
        pass


def _chain_settings(seed):
    rng = np.random.default_rng(seed)
    return {"enabled": True, "filters": [
        {"type": "Peaking", "frequency": float(rng.uniform(300, 3000)), "width": float(rng.uniform(100, 800)), "gain": float(rng.uniform(-9, 9))},
        {"type": "LowPass", "frequency": float(rng.uniform(5000, 12000)), "q": float(rng.uniform(0.5, 1.2)), "passes": 2}]}


def _frames(seed):
    """Per source, the byte frames written in order: 2.5 s of a tone + noise, frames of 0..~0.12 s."""
    rng = np.random.default_rng(seed)
    out = {}
    for src, rate in SOURCES.items():
        t = np.arange(int(rate * 2.5)) / rate
        x = (np.clip(0.4 * np.sin(2 * np.pi * 900 * t) + rng.normal(0, 0.1, t.size), -1, 1) * 32767).astype("<i2").tobytes()
        fr, pos = [], 0
        while pos < len(x):
            r = rng.random()
            n = 0 if r < 0.05 else 1 if r < 0.1 else int(rng.integers(200, rate // 8))
            fr.append(x[pos:pos + 2 * n])
            pos += 2 * n
        out[src] = fr
    return out


def _run(native, frames, processed, monitored, clear_after=None):
    o = S.Orchestrator()
    o.register("b48", _Fake(), SPEC48)
    o.register("p32", _Fake(), SPEC32)
    errors = []
    wb = S.WindowBatcher(o, R.ResultsQueue(size=100000), max_batch=16, clock=lambda: 50.0, native=native,
                         on_error=lambda *a: errors.append(a))
    for src, rate in SOURCES.items():
        wb.allocate(src, "b48", capacity=1 << 17, source_rate=rate)
        wb.allocate(src, "p32", capacity=1 << 17, source_rate=rate)
        if processed:
            wb.set_processing(src, rate, _chain_settings(rate), GAIN_DB)
        if monitored:
            wb.set_sound_level(src, rate, interval_s=INTERVAL[src], name=None if src == "a48" else "mic-b")
    reports = []
    n = max(len(f) for f in frames.values())
    for k in range(n):
        for src, fr in frames.items():
            if k < len(fr):
                wb.write(src, fr[k])
        if k % 3 == 2:
            wb.tick()
        if clear_after is not None and k == clear_after:
            wb.tick()
            reports += wb.take_sound_levels()
            for src in SOURCES:
                wb.clear_sound_level(src)
    while wb.tick():
        pass
    wb.tick()
    reports += wb.take_sound_levels()
    windows = {}
    while wb.queue.qsize():
        msg = wb.queue.get()
        windows.setdefault((msg.model_id, msg.source), []).append(msg.pcm_data)
    assert not errors and wb.errors == 0
    wb.close()
    return reports, windows


def _want(frames, processed, upto=None):
    """The restatement: per source, each non-empty frame (processed as eqref does) one ProcessSamples call."""
    want = {}
    for src, rate in SOURCES.items():
        fr = frames[src][:upto]
        if processed:
            st = {0: eqref.Stream(host.build_filter_chain(_chain_settings(rate), rate), host.gain_linear(GAIN_DB))}
            fr = [b.tobytes() for b in eqref.process(st, [(0, np.frombuffer(f, "<i2")) for f in fr])]
        p = {0: slref.Processor(rate, INTERVAL[src])}
        reps = slref.process(p, [(0, np.frombuffer(f, "<i2")) for f in fr if len(f)], native=True)
        want[src] = [{"timestamp": 50.0, "source": src, "name": src if src == "a48" else "mic-b",
                      "duration_seconds": r["duration_seconds"], "octave_bands": r["octave_bands"]} for r in reps]
    return want


def _by_source(reports):
    out = {src: [] for src in SOURCES}
    for r in reports:
        out[r["source"]].append(r)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("processed", [False, True], ids=["raw", "eq+6dB"])
def test_sound_levels_match_the_restatement(gpu, processed):
    frames = _frames(21)
    _, plain = _run(True, frames, processed, monitored=False)
    want = _want(frames, processed)
    assert all(len(v) >= 1 for v in want.values()) and sum(len(v) for v in want.values()) >= 3
    for native in (True, False):
        got, windows = _run(native, frames, processed, monitored=True)
        assert _by_source(got) == want, native
        assert windows == plain, native                                       # the model windows are untouched by the monitor


@pytest.mark.gpu
@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
def test_clear_sound_level_stops_the_reports(gpu, native):
    frames = _frames(22)
    k = 12
    got, _ = _run(native, frames, True, monitored=True, clear_after=k)
    want = _want(frames, True, upto=k + 1)
    assert _by_source(got) == want
    full = _want(frames, True)
    assert sum(map(len, full.values())) > sum(map(len, want.values()))       # the monitor would have reported more


@pytest.mark.gpu
def test_set_sound_level_again_starts_a_fresh_stream(gpu):
    o = S.Orchestrator()
    o.register("b48", _Fake(), SPEC48)
    wb = S.WindowBatcher(o, R.ResultsQueue(size=1000), clock=lambda: 7.0)
    wb.allocate("s", "b48", capacity=1 << 17)
    rng = np.random.default_rng(2)
    x = rng.integers(-20000, 20000, 48000 * 2).astype("<i2")
    wb.set_sound_level("s", 48000, interval_s=1)
    wb.write("s", x[:30000].tobytes())
    wb.set_sound_level("s", 48000, interval_s=1)                              # a new Processor: the 30 000 samples are gone
    wb.write("s", x[30000:78000].tobytes())
    wb.tick()
    got = wb.take_sound_levels()
    want = slref.process({0: slref.Processor(48000, 1)}, [(0, x[30000:78000])])
    assert [r["octave_bands"] for r in got] == [r["octave_bands"] for r in want] and len(got) == 1
    assert got[0]["timestamp"] == 7.0 and got[0]["name"] == "s" and wb.take_sound_levels() == []
    with pytest.raises(S.StreamError):
        wb.set_sound_level("s", 0)
    wb.close()
