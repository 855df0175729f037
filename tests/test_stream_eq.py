"""WindowBatcher with a source's EQ chain and input gain (set_processing): the analysis route's processing
(AudioRouter.applyProcessing, internal/audiocore/router.go:1006-1080) runs once per frame at the source rate, before the rate
fan-out of BufferConsumer.Write.  Every buffer of a processed source holds the windows of the reference's AnalysisBuffer
(oracle/gostream.py) fed the tests/eqref.py-processed stream (resampled after processing for a 32 kHz model); an unprocessed
source beside it is unchanged; native and Python rings agree."""
import numpy as np
import pytest

import eqref
from birdnet_go_amd import host
from birdnet_go_amd import results as R
from birdnet_go_amd import stream as S
from oracle.gostream import GoAnalysisBuffer

FR = 48000
SPEC48 = S.ModelSpec(48000, 3.0, clip_bytes=9600)         # 100 ms windows, 50 % overlap
SPEC32 = S.ModelSpec(32000, 5.0, clip_bytes=6400)
STOCK = {"enabled": True, "filters": [{"type": "HighPass", "frequency": 100, "q": 0.7, "passes": 0},
                                      {"type": "LowPass", "frequency": 15000, "q": 0.7, "passes": 0}]}
GAIN_DB = 6.0


class _Fake:
    def predict_batch(self, flat, n):
        x = np.asarray(flat, np.float32).reshape(n, -1)
        return [[("sp", float(np.float32(0.5) + x[i, 0]))] for i in range(n)]

    def close(self):
        pass


def _streams(seed):
    rng = np.random.default_rng(seed)
    t = np.arange(FR * 2) / FR
    mk = lambda f: (np.clip(0.45 * np.sin(2 * np.pi * f * t) + 0.2 + rng.normal(0, 0.05, t.size), -1, 1) * 32767).astype("<i2").tobytes()
    return {"eq": mk(700), "plain": mk(1300)}


def _run(models, native, streams, processed=("eq",), seed=8):
    o = S.Orchestrator()
    for m, (spec, _) in models.items():
        o.register(m, _Fake(), spec)
    errors = []
    wb = S.WindowBatcher(o, R.ResultsQueue(size=100000), max_batch=16, clock=lambda: 50.0, native=native,
                         on_error=lambda *a: errors.append(a))
    for s in streams:
        for m, (_, rate) in models.items():
            wb.allocate(s, m, capacity=1 << 16, source_rate=rate)
    for s in processed:
        wb.set_processing(s, FR, STOCK, GAIN_DB)
    rng = np.random.default_rng(seed)
    pos = {s: 0 for s in streams}
    while any(pos[s] < len(b) for s, b in streams.items()):
        for s, b in streams.items():
            r = rng.random()
            n = 0 if r < 0.05 else 1 if r < 0.1 else int(rng.integers(800, 6000))
            wb.write(s, b[pos[s]:pos[s] + 2 * n])
            pos[s] += 2 * n
        wb.tick()
    while wb.tick():
        pass
    wb.tick()
    got = {}
    while wb.queue.qsize():
        msg = wb.queue.get()
        got.setdefault((msg.model_id, msg.source), []).append(msg.pcm_data)
    assert not errors and wb.errors == 0
    return got, wb


def _oracle_windows(data, spec):
    clip, overlap, read = spec.buffer_dimensions()
    g = GoAnalysisBuffer(len(data) + clip, overlap, read)
    g.Write(data)
    out = []
    while True:
        w = g.Read()
        if w is None:
            return out
        out.append(bytes(w))


def _processed(data):
    chain = host.build_filter_chain(STOCK, FR)
    return eqref.process({0: eqref.Stream(chain, host.gain_linear(GAIN_DB))}, [(0, np.frombuffer(data, "<i2"))])[0].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("models", ["b48", "b48+p32"])
def test_processed_source_windows_match_the_oracle(gpu, models):
    streams = _streams(3)
    cfg = {"b48": (SPEC48, FR)}
    if models == "b48+p32":
        cfg["p32"] = (SPEC32, FR)
    alone, wb0 = _run(cfg, True, streams, processed=())
    wb0.close()
    runs = {}
    for native in (True, False):
        got, wb = _run(cfg, native, streams)
        runs[native] = got
        assert list(wb.eq_streams) == ["eq"]
        wb.close()
    assert runs[True] == runs[False]                              # native and Python rings agree
    got = runs[True]
    proc = _processed(streams["eq"])
    assert proc != streams["eq"]
    want48 = _oracle_windows(proc, SPEC48)
    assert len(want48) >= 10 and got[("b48", "eq")] == want48     # processed at 48 kHz, as the reference's route
    if "p32" in cfg:                                              # processed at the source rate, resampled after
        prefix = host.StreamResampler(FR, 32000).resample_into(proc)
        want32 = _oracle_windows(prefix, SPEC32)
        assert len(want32) >= 5 and got[("p32", "eq")] == want32
    for m in cfg:                                                 # the unprocessed source beside it is unchanged
        assert got[(m, "plain")] == alone[(m, "plain")]
    assert got[("b48", "plain")] == _oracle_windows(streams["plain"], SPEC48)


@pytest.mark.gpu
@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
def test_clear_processing_restores_the_raw_path(gpu, native):
    o = S.Orchestrator()
    o.register("b48", _Fake(), SPEC48)
    wb = S.WindowBatcher(o, R.ResultsQueue(size=1000), native=native)
    wb.allocate("a", "b48", capacity=1 << 16)
    b = _streams(4)["eq"]
    wb.set_processing("a", FR, STOCK, GAIN_DB)
    wb.write("a", b[:19200])
    wb.clear_processing("a")                                      # queued frames keep their processing
    assert not wb.eq_streams and not wb.eq_pending
    wb.write("a", b[19200:38400])
    while wb.tick():
        pass
    got = []
    while wb.queue.qsize():
        got.append(wb.queue.get().pcm_data)
    want = _oracle_windows(_processed(b[:19200]) + b[19200:38400], SPEC48)
    assert got == want and len(want) >= 5
    wb.close()
