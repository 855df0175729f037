"""The ragged denoiser (bnhip_denoise_ragged_pcm16 / _device), the ragged chain (bnhip_process_ragged_pcm16) and the chain fused with
the render and the PNG encoder (bnhip_process_spectrogram_png_ragged_pcm16) against the float64 restatement tests/dnref.py, against
the uniform entries clip by clip, and against their own stages called one after another.

Acceptance rule against the restatement (dnref.compare): every sample is equal, except that a sample whose restated |v| + 0.5 lies
within 1e-6 of an integer may differ by 1 LSB; the excused share of a burst, over all of its clips, is capped at 1e-4 and the cap is
asserted on the restatement before the device output is looked at.  Everything else is byte for byte.

Bursts (tests/dnraggedcases.py) hold the smallest lengths at which each per-clip mechanism can go wrong."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import dncases
import dnraggedcases as rc
import dnref
from birdnet_go_amd import host, loudness, process, spectrogram as sg

from test_parity_gpu import _DevBuf
from test_spectrogram_ref import decode_png

pytestmark = pytest.mark.gpu
RATE = rc.RATE
NR, NF = rc.NR_DB, rc.NF_DB
WIDTH = 64


@functools.lru_cache(maxsize=None)
def run(name):
    """The device's output for a burst, the clips one after another: rendered once, shared, read-only."""
    out = host.denoise_ragged(rc.clips(name), rc.frame(name), NR, NF)
    assert [o.size for o in out] == list(rc.BURSTS[name][1])
    y = np.concatenate(out)
    y.setflags(write=False)
    return y


def split(name, packed):
    return host.ragged_unpack(packed, rc.BURSTS[name][1])


@pytest.mark.parametrize("name", list(rc.BURSTS))
def test_every_clip_meets_the_restatement(gpu, name):
    share = dnref.compare(run(name), None, rc.frame(name), NR, NF, restated=rc.restated(name))
    print(f"{name}: excused share {share:.3g}")


@pytest.mark.parametrize("name", list(rc.BURSTS))
def test_every_clip_equals_the_uniform_entry_on_it_alone(gpu, name):
    clips, got = rc.clips(name), split(name, run(name))
    pick = range(len(clips)) if name != "many" else sorted(set(range(0, len(clips), 7)) | {0, len(clips) - 1})
    for i in pick:
        assert np.array_equal(host.denoise(clips[i], rc.frame(name), NR, NF)[0], got[i]), (i, clips[i].size)


def test_equal_lengths_equal_the_uniform_batch(gpu):
    clips = rc.burst_clips((5197,) * 3)
    got = host.denoise_ragged(clips, 1024, NR, NF)
    assert np.array_equal(np.stack(got), host.denoise(np.stack(clips), 1024, NR, NF))


def test_device_entry_equals_the_host_entry(gpu):
    """The output buffer is poisoned and followed by a guard: a write past a clip's end lands in the next clip or in the guard."""
    name, guard = "tiles", 256
    N, lens = rc.BURSTS[name]
    x, lens32 = host.ragged_pack(rc.clips(name))
    ws_bytes = host.denoise_ragged_workspace_size(lens, N)
    d_in, d_out, d_ws = _DevBuf(x.nbytes), _DevBuf(x.nbytes + guard), _DevBuf(ws_bytes)
    try:
        d_in.upload(x)
        d_out.upload(np.full(x.nbytes + guard, 0x55, np.uint8))
        host.denoise_ragged_device(d_in.ptr, lens32, N, NR, NF, d_out.ptr, d_ws.ptr, ws_bytes)
        raw = d_out.download((x.nbytes + guard,), np.uint8)       # (the null stream orders the copy after the kernel)
    finally:
        for d in (d_in, d_out, d_ws):
            d.free()
    assert (raw[x.nbytes:] == 0x55).all()
    assert np.array_equal(raw[:x.nbytes].view(np.int16), run(name))


@pytest.mark.parametrize("name", ["tiles", "rounds"])
def test_no_reduction_is_the_identity(gpu, name):
    """Independent of the restatement: nr_db = 0 makes every gain 1, and the output is the input."""
    clips = rc.clips(name)
    for got, want in zip(host.denoise_ragged(clips, rc.frame(name), 0.0, -40.0), clips):
        assert np.array_equal(got, want), want.size


# ------------------------------------------------------------------------------------------------ the chain
def _records(res):
    return [tuple(getattr(r, f) for f, _ in host.Loudness._fields_) for r in res]


CHAIN_SETS = [(1024, False, 0.0), (1024, True, 0.0), (0, True, -7.5)]
CHAIN_IDS = ["denoise", "denoise+normalise", "normalise+gain"]
ALL_STAGES = dict(frame=1024, nr_db=NR, nf_db=NF, normalize=True, target_lufs=-23.0, true_peak_dbtp=-2.0, gain_db=2.0)


def chain_clips():
    return rc.burst_clips(rc.CHAIN_LENS)


@functools.lru_cache(maxsize=None)
def chain_run(frame, normalize, gain_db):
    return host.process_ragged(chain_clips(), RATE, frame, NR, NF, normalize, -23.0, -2.0, gain_db)


@pytest.mark.parametrize("frame,normalize,gain_db", CHAIN_SETS, ids=CHAIN_IDS)
def test_ragged_chain_equals_its_ragged_stages_one_after_another(gpu, frame, normalize, gain_db):
    got, got_res = chain_run(frame, normalize, gain_db)
    want, want_res = chain_clips(), None
    if frame:
        want = host.denoise_ragged(want, frame, NR, NF)
    if normalize:
        want_res, want = host.loudness_normalize_ragged(want, RATE, -23.0, -2.0, math.inf, False)
    if gain_db:
        want = [dnref.quant(w.astype(np.float64) * loudness.factor_from_db(gain_db)) for w in want]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), i
    assert (got_res is None) == (want_res is None)
    if normalize:
        assert _records(got_res) == _records(want_res)
        assert any(r.factor != 1.0 for r in got_res)


@pytest.mark.parametrize("frame,normalize,gain_db", CHAIN_SETS, ids=CHAIN_IDS)
def test_ragged_chain_equals_the_uniform_chain_per_clip(gpu, frame, normalize, gain_db):
    got, got_res = chain_run(frame, normalize, gain_db)
    for i, clip in enumerate(chain_clips()):
        want, want_res = host.process(clip, RATE, frame, NR, NF, normalize, -23.0, -2.0, gain_db)
        assert np.array_equal(got[i], want[0]), i
        if normalize:
            assert _records([got_res[i]]) == _records(want_res), i


# ------------------------------------------------------------------------------------------------ the fused entry
@functools.lru_cache(maxsize=None)
def processed():
    """(clips, records) of the chain's burst with all three stages: what the fused entry's render starts from."""
    return host.process_ragged(chain_clips(), RATE, **ALL_STAGES)


@pytest.mark.parametrize("rate_out", [0, 12000])
def test_fused_entry_equals_the_chain_then_the_render(gpu, tmp_path, rate_out):
    pal = sg.palette("default")
    pcm, res = processed()
    want = host.spectrogram_png_ragged(pcm, RATE, WIDTH, pal, rate_out=rate_out)
    png, got_res, got_pcm = host.process_spectrogram_png_ragged(chain_clips(), RATE, WIDTH, pal, rate_out=rate_out, want_pcm=True, **ALL_STAGES)
    assert len(png) == len(want) == len(rc.CHAIN_LENS)
    for i in range(len(want)):
        assert png[i] == want[i], i
        assert np.array_equal(got_pcm[i], pcm[i]), i
    assert _records(got_res) == _records(res)
    assert any(r.factor != 1.0 for r in got_res)
    # without out_pcm the files are the same
    png2, res2, none = host.process_spectrogram_png_ragged(chain_clips(), RATE, WIDTH, pal, rate_out=rate_out, **ALL_STAGES)
    assert none is None and png2 == png and _records(res2) == _records(res)
    # one file decodes to the render of the processed clip
    img = host.spectrogram_ragged(pcm, RATE, WIDTH, rate_out=rate_out)
    path = tmp_path / "clip4.png"
    path.write_bytes(png[4])
    pix, got_pal = decode_png(str(path))
    assert np.array_equal(pix, img[4]) and np.array_equal(got_pal, pal)


def test_fused_entry_out_cap_one_byte_short(gpu):
    lib = host.load_library()
    x, lens = host.ragged_pack(chain_clips())
    pal = np.ascontiguousarray(sg.palette("default"), np.uint8).reshape(-1)
    height, _ = host.spectrogram_size(WIDTH)
    cap = host.png_max_bytes(lens.size, WIDTH, height)
    out, offs = np.full(cap, 0x55, np.uint8), np.zeros(lens.size + 1, np.uint64)
    res = (host.Loudness * lens.size)()
    ci, cd, vp = C.c_int, C.c_double, C.c_void_p
    rc_ragged = lib.bnhip_spectrogram_png_ragged_pcm16(ci(0), vp(x.ctypes.data), ci(lens.size), vp(lens.ctypes.data), ci(RATE), ci(0), ci(WIDTH),
                                                       ci(height), vp(), cd(0.0), cd(100.0), vp(pal.ctypes.data), vp(out.ctypes.data),
                                                       C.c_size_t(cap - 1), vp(offs.ctypes.data))
    msg_ragged = lib.bnhip_last_error()
    rc_fused = lib.bnhip_process_spectrogram_png_ragged_pcm16(ci(0), vp(x.ctypes.data), ci(lens.size), vp(lens.ctypes.data), ci(RATE), ci(1024),
                                                              cd(NR), cd(NF), ci(1), cd(-23.0), cd(-2.0), cd(2.0), ci(0), ci(WIDTH), ci(height),
                                                              vp(), cd(0.0), cd(100.0), vp(pal.ctypes.data), vp(out.ctypes.data),
                                                              C.c_size_t(cap - 1), vp(offs.ctypes.data), vp(C.addressof(res)), vp())
    assert rc_fused == rc_ragged == host.E_INVALID and lib.bnhip_last_error() == msg_ragged
    assert (out == 0x55).all() and not offs.any()


# ------------------------------------------------------------------------------------------------ the Python surface
def test_python_surface(gpu, tmp_path):
    clips = chain_clips()
    pcm, reports = process.process_clips(clips, RATE, denoise="medium", normalize=True, gain_db=2.0, ragged=True)
    want, want_res = processed()
    assert all(np.array_equal(a, b) for a, b in zip(pcm, want)) and len(pcm) == len(want) and _records(reports) == _records(want_res)
    den = process.denoise_clips(clips, RATE, preset="medium", ragged=True)
    assert all(np.array_equal(a, b) for a, b in zip(den, host.denoise_ragged(clips, 1024, NR, NF)))
    # an equal-length batch: the fused call returns and writes what the two calls do
    x = np.stack([dncases.signal(s, RATE) for s in ("tone_noise", "chirp")])
    two = [str(tmp_path / f"two{i}.png") for i in range(2)]
    one = [str(tmp_path / f"one{i}.png") for i in range(2)]
    idx2 = process.processed_spectrogram(x, two, WIDTH, RATE, denoise="medium", normalize=True, gain_db=2.0)
    idx1 = process.processed_spectrogram(x, one, WIDTH, RATE, denoise="medium", normalize=True, gain_db=2.0, fused=True)
    assert np.array_equal(idx1, idx2)
    for a, b in zip(one, two):
        assert open(a, "rb").read() == open(b, "rb").read()
    # a ragged list: one decodable file per clip, the render of the processed clip
    paths = [str(tmp_path / f"r{i}.png") for i in range(len(clips))]
    idx = process.processed_spectrogram(clips, paths, WIDTH, RATE, denoise="medium", normalize=True, gain_db=2.0, fused=True)
    kw = sg._render_args(RATE, WIDTH, None, "default", "100")
    img = host.spectrogram_ragged(want, RATE, WIDTH, **kw)
    assert np.array_equal(idx, img)
    for i, p in enumerate(paths):
        pix, pal = decode_png(p)
        assert np.array_equal(pix, img[i]) and np.array_equal(pal, sg.palette("default"))
