"""The device denoiser (bnhip_denoise_pcm16 / bnhip_denoise_device) and the processed-audio chain (bnhip_process_pcm16) against the
float64 restatement of the spec, tests/dnref.py.

Acceptance rule (dnref.compare): every sample is equal, except that a sample whose restated |v| + 0.5 lies within 1e-6 of an
integer may differ by 1 LSB; the excused share of a case, over all of its clips, is capped at 1e-4 and the cap is asserted on
the restatement before the device output is looked at.  (The device's and numpy's transforms differ by about 1e-11 LSB.)

Shapes (tests/dncases.py) are the smallest at which each mechanism can go wrong: every frame length's pass structure, many
tiles with a partial last tile and a partial last hop, a clip of exactly 16 hops, clips below one hop, an odd clip count."""
import ctypes as C
import math

import numpy as np
import pytest

import dncases
import dnref
from birdnet_go_amd import host, loudness, process, spectrogram as sg

from test_parity_gpu import _DevBuf
from test_spectrogram_ref import decode_png

pytestmark = pytest.mark.gpu
RATE = dncases.RATE


def run(case):
    return host.denoise(dncases.clips(case), *dncases.params(case))


@pytest.mark.parametrize("case", list(dncases.CASES))
def test_device_matches_the_restatement(gpu, case):
    dev = run(case)
    share = dnref.compare(dev, dncases.clips(case), *dncases.params(case), restated=dncases.restated(case))
    print(f"{case}: excused share {share:.3g}")


@pytest.mark.parametrize("N,n", [(64, 5000), (256, 4099), (2048, 6 * 2048 + 5)])
def test_no_reduction_is_the_identity(gpu, N, n):
    """Independent of the restatement: nr_db = 0 makes every gain 1, and the output is the input."""
    x = np.stack([dncases.signal(s, n) for s in ("noise_full", "chirp", "tone_noise")])
    assert np.array_equal(host.denoise(x, N, 0.0, -40.0), x)


def test_a_clip_under_the_floor_leaves_at_the_gain_floor(gpu):
    """Independent of the restatement: noise_33 at medium lies under the floor in every bin, so out = round(g_min pcm)."""
    x = dncases.signal("noise_33", dncases.PRESET_LEN)
    want = dnref.quant(10.0 ** (-12.0 / 20.0) * x.astype(np.float64))
    assert np.array_equal(host.denoise(x, dncases.PRESET_N, 12.0, -40.0)[0], want)


@pytest.mark.parametrize("case", ["tiles_many", "preset_medium"])
def test_a_clip_does_not_depend_on_its_batch(gpu, case):
    batch = run(case)
    N, nr, nf = dncases.params(case)
    for i, clip in enumerate(dncases.clips(case)):
        assert np.array_equal(host.denoise(clip, N, nr, nf)[0], batch[i]), i


def test_device_entry_equals_the_host_entry(gpu):
    case = "tiles_many"
    x = dncases.clips(case)
    N, nr, nf = dncases.params(case)
    B, n = x.shape
    ws_bytes = host.denoise_workspace_size(B, n, N)
    d_in, d_out, d_ws = _DevBuf(x.nbytes), _DevBuf(x.nbytes), _DevBuf(ws_bytes)
    try:
        d_in.upload(x)
        host.denoise_device(d_in.ptr, B, n, N, nr, nf, d_out.ptr, d_ws.ptr, ws_bytes)
        got = d_out.download(x.shape, np.int16)           # (the null stream orders the copy after the kernel)
    finally:
        for d in (d_in, d_out, d_ws):
            d.free()
    assert np.array_equal(got, run(case))


def _records(res):
    return [tuple(getattr(r, f) for f, _ in host.Loudness._fields_) for r in res]


@pytest.mark.parametrize("frame,normalize,gain_db", [(1024, False, 0.0), (1024, True, 0.0), (0, True, -7.5)],
                         ids=["denoise", "denoise+normalise", "normalise+gain"])
def test_chain_equals_its_stages_one_after_another(gpu, frame, normalize, gain_db):
    """bnhip_process_pcm16 against bnhip_denoise_pcm16, bnhip_loudness_normalize_pcm16(-23, -2, no clamp, no fallback) and the
    saturating int16 gain called one after another: bytes and records."""
    x = np.stack([dncases.signal(s, RATE) for s in ("tone_noise", "chirp", "noise_330")])          # 1 s: ten loudness sub-blocks
    got, got_res = host.process(x, RATE, frame, 12.0, -40.0, normalize, -23.0, -2.0, gain_db)
    want, want_res = x, None
    if frame:
        want = host.denoise(want, frame, 12.0, -40.0)
    if normalize:
        want_res, want = host.loudness_normalize(want, RATE, -23.0, -2.0, math.inf, False)
    if gain_db:
        want = dnref.quant(want.astype(np.float64) * loudness.factor_from_db(gain_db))
    assert np.array_equal(got, want)
    assert (got_res is None) == (want_res is None)
    if normalize:
        assert _records(got_res) == _records(want_res)
        assert any(r.factor != 1.0 for r in got_res)


def test_python_surface(gpu, tmp_path):
    x = np.stack([dncases.signal(s, RATE) for s in ("tone_noise", "chirp")])
    pcm, reports = process.process_clips(x, RATE, denoise="medium", normalize=True, gain_db=2.0)
    want, want_res = host.process(x, RATE, process.frame_for_rate(RATE), 12.0, -40.0, True, -23.0, -2.0, 2.0)
    assert np.array_equal(pcm, want) and _records(reports) == _records(want_res)
    assert np.array_equal(process.denoise_clips(x, RATE, preset="heavy"), host.denoise(x, 1024, 20.0, -50.0))
    assert np.array_equal(process.denoise_clips(x, RATE, preset="", nr_db=6, nf_db=-30, frame=256), host.denoise(x, 256, 6.0, -30.0))
    # the processed spectrogram: PNG files that decode to the render of the processed PCM
    paths = [str(tmp_path / f"{i}.png") for i in range(2)]
    width = 64
    idx = process.processed_spectrogram(x, paths, width, RATE, denoise="medium", normalize=True, gain_db=2.0)
    kw = sg._render_args(RATE, width, None, "default", "100")
    img = host.spectrogram(pcm, RATE, width, **kw)
    assert np.array_equal(idx, img)
    for i, p in enumerate(paths):
        pix, pal = decode_png(p)
        assert np.array_equal(pix, img[i]) and np.array_equal(pal, sg.palette("default"))
