"""FLAC on the device (bnhip_flac_*, bnhip_loudness_flac_pcm16) against the numpy restatement of the spec (tests/flacref.py) and an
independent decoder (tests/flacdec.py).

Acceptance: the encoder is integer arithmetic, so every byte and every offset equals the restatement's; the decoder returns the
gained input (the gain restated by loudref.apply_gain); the device entry equals the host entry; the fused entry equals
bnhip_loudness_normalize_pcm16 followed by bnhip_flac_encode_pcm16, records and bytes.  The cases (tests/flaccases.py) run as
batches of 1, 3 and 65 clips."""
import os

import numpy as np
import pytest

import flaccases as K
import flacdec
import flacref
from birdnet_go_amd import flac, host, loudness

from test_parity_gpu import _DevBuf

pytestmark = pytest.mark.gpu
EXPORT = dict(T=-23.0, C=-1.0, max_gain=60.0, gate_fallback=True)        # actions_database.go:1392-1438
UPLOAD = dict(T=-23.0, C=-1.0, max_gain=30.0, gate_fallback=False)       # encode_native.go:25-66


def first_difference(a, b):
    a, b = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    m = min(a.size, b.size)
    d = np.flatnonzero(a[:m] != b[:m])
    return (int(d[0]) if d.size else m), a.size, b.size


@pytest.mark.parametrize("name", list(K.CASES))
def test_bytes_and_offsets_equal_the_restatement(gpu, name):
    rate, clips, factor, seek = K.CASES[name]
    want, want_off, _, gained = K.reference(name)
    got, off = host.flac_encode(clips, rate, factor, seek, raw=True)
    assert off.tolist() == want_off.tolist(), name
    assert got.tobytes() == want, (name, first_difference(got.tobytes(), want))
    assert int(off[-1]) <= host.flac_max_bytes(len(clips), clips.shape[1], seek)
    for c in range(min(len(clips), 4)):                                  # (the restatement's own streams decode in test_flac_ref.py)
        y, info = flacdec.decode(got[int(off[c]):int(off[c + 1])].tobytes())
        assert np.array_equal(y, gained[c]) and info["rate"] == rate, (name, c)


@pytest.mark.parametrize("name", ["contents_one_clip", "len257", "len8225", "sixty_five"])
def test_device_entry_equals_the_host_entry(gpu, name):
    rate, clips, factor, seek = K.CASES[name]
    Bc, n = clips.shape
    want, want_off = host.flac_encode(clips, rate, factor, seek, raw=True)
    cap, ws = host.flac_max_bytes(Bc, n, seek), host.flac_workspace_size(Bc, n)
    bufs = d_in, d_fac, d_out, d_off, d_ws = _DevBuf(clips.nbytes), _DevBuf(8 * Bc), _DevBuf(cap), _DevBuf(8 * (Bc + 1)), _DevBuf(ws)
    try:
        d_in.upload(np.ascontiguousarray(clips))
        if factor is not None:
            d_fac.upload(np.ascontiguousarray(factor, np.float64))
        host.flac_encode_device(d_in.ptr, Bc, n, rate, d_out.ptr, cap, d_off.ptr, d_ws.ptr, ws, d_fac.ptr if factor is not None else None, seek)
        off = d_off.download((Bc + 1,), np.uint64)                       # (a blocking copy on the null stream: after the kernels)
        out = d_out.download((cap,), np.uint8)
    finally:
        for b in bufs:
            b.free()
    assert off.tolist() == want_off.tolist() and out[:int(off[-1])].tobytes() == want.tobytes()


def loud_batch(rate, n, count):
    """Tones and noises of several levels, a sub-gate clip and silence: plans with gain, clamp, lift and none."""
    rng = np.random.default_rng(77)
    t = np.arange(n)
    rows = []
    for i in range(count):
        amp = (0.6, 0.02, 0.0004, 0.2, 0.0)[i % 5]
        x = amp * 32767.0 * (np.sin(2.0 * np.pi * (200.0 + 90.0 * i) * t / rate) if i % 2 == 0 else rng.standard_normal(n) / 3.0)
        rows.append(np.clip(np.round(x), -32768, 32767).astype(np.int16))
    return np.stack(rows)


def fields(res):
    return [tuple(getattr(g, f) for f, _ in host.Loudness._fields_) for g in res]


@pytest.mark.parametrize("rate,n,count,plan,seek", [(8000, 5 * 800 + 37, 5, EXPORT, 8000), (8000, 5 * 800 + 37, 5, UPLOAD, 0),
                                                    (48000, 5 * 4800 + 4799, 3, EXPORT, 48000), (48000, 5 * 4800 + 4799, 3, UPLOAD, 0)])
def test_fused_entry_equals_normalize_then_encode(gpu, rate, n, count, plan, seek):
    clips = loud_batch(rate, n, count)
    res, streams = host.loudness_flac(clips, rate, plan["T"], plan["C"], plan["max_gain"], plan["gate_fallback"], seek)
    want_res, pcm = host.loudness_normalize(clips, rate, plan["T"], plan["C"], plan["max_gain"], plan["gate_fallback"])
    assert fields(res) == fields(want_res)
    assert any(g.gain_db != 0.0 for g in res)
    assert streams == host.flac_encode(pcm, rate, None, seek)
    for s, y in zip(streams, pcm):
        assert np.array_equal(flacdec.decode(s)[0], y)


def test_normalize_and_encode_groups_a_burst_by_length(gpu):
    a, b = loud_batch(8000, 5 * 800 + 37, 3), loud_batch(8000, 4 * 800, 2)
    burst = [a[0], b[1], a[1], b[0], a[2]]
    res, streams = flac.normalize_and_encode(burst, 8000, max_gain_db=loudness.EXPORT_MAX_GAIN_DB, gate_fallback=True, seek_interval=8000)
    ra, sa = host.loudness_flac(a, 8000, -23.0, -1.0, 60.0, True, 8000)
    rb, sb = host.loudness_flac(b, 8000, -23.0, -1.0, 60.0, True, 8000)
    assert fields(res) == fields([ra[0], rb[1], ra[1], rb[0], ra[2]])
    assert streams == [sa[0], sb[1], sa[1], sb[0], sa[2]]
    gains = [None, -6.0, 0.0, 3.5, 0.0]
    enc = flac.encode_clips(burst, 8000, gain_db=[0.0 if g is None else g for g in gains])
    for s, x, g in zip(enc, burst, gains):
        assert s == flacref.encode_batch([x], 8000, None if g is None else [loudness.factor_from_db(g)])[0]


def test_tawny_owl_is_identical_to_the_restatement_and_smaller_than_pcm(gpu):
    """The reference's own recording (48 kHz, five 3 s clips), reduced to 16 bits: the first 40 frames."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tawnyowl_pcm32.npz"))
    acc = np.cumsum(z["delta"].astype(np.int64))
    pcm = (((acc + 2**31) % 2**32 - 2**31) >> 16).astype(np.int16)[:40 * 4096]
    got = host.flac_encode(pcm, 48000)[0]
    assert got == flacref.encode(pcm, 48000)
    ratio = len(got) / (2.0 * pcm.size)
    print(f"tawny owl, 40 frames at 16 bits: {len(got)} bytes, {ratio:.4f} of the PCM")
    assert ratio < 1.0
