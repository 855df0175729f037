"""WindowBatcher with models at two rates on the same 48 kHz sources: BufferConsumer.Write's rate groups
(internal/analysis/buffer_consumer.go:105-210).  The 48 kHz model sees exactly what it sees alone; a 32 kHz model's windows are
those of the reference's AnalysisBuffer (oracle/gostream.py) fed the resampled stream; the native and Python rings agree."""
import numpy as np
import pytest

from birdnet_go_amd import host
from birdnet_go_amd import results as R
from birdnet_go_amd import stream as S
from oracle.gostream import GoAnalysisBuffer

FR = 48000
SPEC48 = S.ModelSpec(48000, 3.0, clip_bytes=9600)         # 100 ms windows, 50 % overlap
SPEC32 = S.ModelSpec(32000, 5.0, clip_bytes=6400)
SPEC32B = S.ModelSpec(32000, 5.0, clip_bytes=10000)


class _Fake:
    def predict_batch(self, flat, n):
        x = np.asarray(flat, np.float32).reshape(n, -1)
        return [[("sp", float(np.float32(0.5) + x[i, 0]))] for i in range(n)]

    def close(self):
        pass


def _streams(n_src, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(FR * 2) / FR
    return {f"src{i}": (np.clip(0.4 * np.sin(2 * np.pi * (600 + 91 * i) * t) + rng.normal(0, 0.05, t.size), -1, 1) * 32767)
            .astype("<i2").tobytes() for i in range(n_src)}


def _run(models, native, streams, seed=8):
    """models: {model_id: (spec, source_rate or None)} -> {(model_id, source): [pcm bytes of each window]} (and the batcher)."""
    o = S.Orchestrator()
    for m, (spec, _) in models.items():
        o.register(m, _Fake(), spec)
    wb = S.WindowBatcher(o, R.ResultsQueue(size=100000), max_batch=16, clock=lambda: 50.0, native=native)
    for s in streams:
        for m, (_, rate) in models.items():
            wb.allocate(s, m, capacity=1 << 16, source_rate=rate)
    rng = np.random.default_rng(seed)
    pos = {s: 0 for s in streams}
    while any(pos[s] < len(b) for s, b in streams.items()):
        for s, b in streams.items():
            r = rng.random()
            n = 0 if r < 0.05 else 1 if r < 0.1 else int(rng.integers(1, 40)) * 2 + 1 if r < 0.2 else int(rng.integers(800, 6000))
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


@pytest.mark.gpu
@pytest.mark.parametrize("two_32k", [False, True], ids=["one32k", "two32k"])
def test_models_at_two_rates_on_48k_sources(gpu, two_32k):
    streams = _streams(8, 21)
    models = {"b48": (SPEC48, FR), "p32": (SPEC32, FR)}
    if two_32k:
        models["q32"] = (SPEC32B, FR)
    alone, wb0 = _run({"b48": (SPEC48, None)}, True, streams)
    runs = {}
    for native in (True, False):
        got, wb = _run(models, native, streams)
        runs[native] = got
        if native:                                               # one bank for the pair, one stream per source: resampled once
            assert list(wb.banks) == [(FR, 32000)] and len(wb.bank_streams) == len(streams)
        else:
            assert len(wb.resamplers) == len(streams)
        wb.close()
    wb0.close()
    assert runs[True] == runs[False]                             # native and Python rings agree
    got = runs[True]
    for s, b in streams.items():
        assert got[("b48", s)] == alone[("b48", s)] and len(got[("b48", s)]) >= 10   # the 48 kHz model as if alone
        prefix = host.StreamResampler(FR, 32000).resample_into(b)                   # what the stream determines so far
        assert prefix == host.Resampler(FR, 32000).resample_to(b)[:len(prefix)]
        for m, (spec, _) in models.items():
            if m == "b48":
                continue
            want = _oracle_windows(prefix, spec)
            assert len(want) >= 5 and got[(m, s)] == want, (m, s)


@pytest.mark.gpu
@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
def test_remove_frees_the_stream_and_reallocation_starts_fresh(gpu, native):
    o = S.Orchestrator()
    o.register("p32", _Fake(), SPEC32)
    wb = S.WindowBatcher(o, R.ResultsQueue(size=1000), native=native)
    b = _streams(1, 4)["src0"]
    wb.allocate("a", "p32", capacity=1 << 16, source_rate=FR)
    wb.write("a", b[:20000])
    wb.tick()
    wb.remove("a")
    assert not wb.rates and not wb.resamplers and not wb.bank_streams and not any(wb.pending.values())
    wb.allocate("a", "p32", capacity=1 << 16, source_rate=FR)
    wb.write("a", b[20000:60000])
    while wb.tick():
        pass
    wb.tick()
    got = []
    while wb.queue.qsize():
        got.append(wb.queue.get().pcm_data)
    want = _oracle_windows(host.StreamResampler(FR, 32000).resample_into(b[20000:60000]), SPEC32)
    assert got[-len(want):] == want and len(want) >= 2
    wb.close()


def test_same_rate_source_is_unchanged():
    """source_rate equal to the model's rate (or None) is today's path: no resampler, the bytes as they are."""
    o = S.Orchestrator()
    o.register("b48", _Fake(), SPEC48)
    for native in (True, False):
        wb = S.WindowBatcher(o, R.ResultsQueue(size=1000), native=native)
        wb.allocate("a", "b48", source_rate=FR)
        wb.allocate("c", "b48")
        assert not wb.rates and not wb.resamplers and not wb.banks
        with pytest.raises(S.StreamError):
            wb.allocate("d", "b48", source_rate=0)
        wb.close()
