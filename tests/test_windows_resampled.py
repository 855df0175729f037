"""bnhip_windows_write_resampled: BufferConsumer.Write's non-native rate group (internal/analysis/buffer_consumer.go:184-210) for
every source of a tick at once.  Held against a second assembler fed per source by the single-stream resampler and
bnhip_windows_write, one write per frame: the collected rows, the source order and the per-source write / overwrite counters
are byte-for-byte the same."""
import numpy as np
import pytest

from birdnet_go_amd import host
from birdnet_go_amd import stream as S
from birdnet_go_amd import synth_model as sm

FR = 48000


def _sources(n_src, n_samples, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n_samples) / FR
    out = []
    for i in range(n_src):
        x = 0.4 * np.sin(2 * np.pi * (500 + 37 * i) * t + i) + rng.normal(0, 0.05, n_samples)
        out.append((np.clip(x, -1, 1) * 32767).astype("<i2"))
    return out


def _run_both(overlap, read, to, n_src, ticks, capacity, on_tick, seed=3):
    """Feeds n_src 48 kHz sources ~100 ms frames for `ticks` ticks into assembler A through one write_resampled per tick and into
    assembler B through a StreamResampler + write per source; on_tick(wa, wb, sa, sb) after every tick."""
    rng = np.random.default_rng(seed)
    frame = FR // 10
    srcs = _sources(n_src, frame * ticks + 64 * ticks, seed)
    wa, wb = S.NativeWindows(overlap, read, max_batch=n_src), S.NativeWindows(overlap, read, max_batch=n_src)
    sa = [wa.add_source(f"s{i}", capacity) for i in range(n_src)]
    sb = [wb.add_source(f"s{i}", capacity) for i in range(n_src)]
    bank = host.ResamplerBank(FR, to, max_streams=n_src)
    st = [bank.add_stream() for _ in range(n_src)]
    rs = [host.StreamResampler(FR, to) for _ in range(n_src)]
    pos = [0] * n_src
    for _ in range(ticks):
        items = []
        for i in range(n_src):
            n = frame + int(rng.integers(-64, 64))
            items.append((st[i], sa[i], srcs[i][pos[i]:pos[i] + n].tobytes()))
            wb.write(sb[i], rs[i].resample_into(srcs[i][pos[i]:pos[i] + n].tobytes()))
            pos[i] += n
        bank.write_windows(wa, items)
        on_tick(wa, wb, sa, sb)
    for i in range(n_src):
        assert wa.stats(sa[i]) == wb.stats(sb[i])
    for r in rs:
        r.close()
    bank.close()
    return wa, wb


@pytest.mark.gpu
def test_write_resampled_equals_per_source_resamplers_perch_geometry(gpu):
    """256 sources at 48 kHz, Perch geometry (32 kHz x 5 s, 50 % overlap), ~100 ms frames, several windows per source."""
    spec = S.ModelSpec(32000, 5.0)
    clip, overlap, read = spec.buffer_dimensions()
    n_windows = [0]

    def on_tick(wa, wb, sa, sb):
        ia, ra = wa.collect()
        ib, rb = wb.collect()
        assert ia == ib                                              # same source order (the tables were filled alike)
        assert np.array_equal(ra, rb)
        n_windows[0] += len(ia)

    wa, wb = _run_both(overlap, read, 32000, 256, 110, 2 * clip, on_tick)
    assert n_windows[0] >= 256 * 3
    wa.close()
    wb.close()


@pytest.mark.gpu
def test_write_resampled_then_predict_topk_tiny_perch(gpu):
    """The clip geometry of the tiny Perch-style model (32 kHz, 8000 samples): bnhip_windows_predict_topk on both assemblers gives
    identical confidences, indices and sources."""
    cfg = sm.tiny_perch_config()
    clf = host.HipClassifier(sm.build_model(cfg), device=0, max_batch=64)
    clip = cfg.n_samples * 2
    overlap, read = clip // 2, clip - clip // 2
    calls = [0]

    def on_tick(wa, wb, sa, sb):
        a = wa.predict_topk(clf, 16, 10, 1)
        b = wb.predict_topk(clf, 16, 10, 1)
        assert a[0] == b[0]
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
        calls[0] += len(a[0])

    wa, wb = _run_both(overlap, read, cfg.sample_rate, 64, 12, 4 * clip, on_tick, seed=5)
    assert calls[0] >= 64 * 4
    wa.close()
    wb.close()
    clf.close()
