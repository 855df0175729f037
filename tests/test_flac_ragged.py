"""FLAC of a ragged burst on the device (bnhip_flac_ragged_*, bnhip_loudness_flac_ragged_pcm16) against the per-clip restatement of
the spec (tests/flacref.py, tests/flaclpcref.py) and the independent decoder (tests/flaclpcdec.py).

Acceptance: a clip's stream depends on that clip alone, so stream c of a burst equals the restatement of clip c byte for byte and
the offsets are the running sum of those lengths; the ragged entry equals the uniform entry on a burst of one length; the device
entry equals the host entry; the fused entry equals ragged normalise followed by ragged encode, records and bytes; the Python
surfaces return the same with ragged=True and ragged=False.  The bursts are tests/raggedcases.py's."""
import numpy as np
import pytest

import flaclpcdec
import raggedcases as K
from birdnet_go_amd import flac, host, loudness

from test_flac import fields, first_difference
from test_parity_gpu import _DevBuf

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("with_factor", [False, True])
@pytest.mark.parametrize("seek", K.SEEKS)
@pytest.mark.parametrize("lpc_order", K.LPC_ORDERS)
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_every_stream_equals_the_restatement_of_its_clip(gpu, name, lpc_order, seek, with_factor):
    clips = K.burst(name)
    want, gained = K.flac_reference(name, lpc_order, seek, with_factor)
    got, off = host.flac_encode_ragged(clips, K.RATE, K.factors(name) if with_factor else None, seek, raw=True, lpc_order=lpc_order)
    assert off.dtype == np.uint64 and off.size == len(clips) + 1 and off[0] == 0
    for c, w in enumerate(want):
        g = got[int(off[c]):int(off[c + 1])].tobytes()
        assert g == w, (name, c, first_difference(g, w))
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert int(off[-1]) == got.size <= host.flac_ragged_max_bytes([c.size for c in clips], seek)
    for c in (0, len(clips) // 2, len(clips) - 1):
        y, info = flaclpcdec.decode(got[int(off[c]):int(off[c + 1])].tobytes())
        assert np.array_equal(y, gained[c]) and info["rate"] == K.RATE, (name, c)


@pytest.mark.parametrize("lpc_order", [0, 8])
def test_one_length_equals_the_uniform_entry(gpu, lpc_order):
    clips = K.burst("c")
    fac = K.factors("c")
    got, off = host.flac_encode_ragged(clips, K.RATE, fac, 8000, raw=True, lpc_order=lpc_order)
    want, want_off = host.flac_encode(np.stack(clips), K.RATE, fac, 8000, raw=True, lpc_order=lpc_order)
    assert off.tolist() == want_off.tolist() and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("lpc_order", [0, 8])
def test_device_entry_equals_the_host_entry(gpu, lpc_order):
    clips = K.burst("a")
    fac = K.factors("a")
    packed, lens = host.ragged_pack(clips)
    B = len(clips)
    want, want_off = host.flac_encode_ragged(clips, K.RATE, fac, 8000, raw=True, lpc_order=lpc_order)
    cap, ws = host.flac_ragged_max_bytes(lens, 8000), host.flac_ragged_workspace_size(lens, lpc_order)
    bufs = d_in, d_fac, d_out, d_off, d_ws = _DevBuf(packed.nbytes), _DevBuf(8 * B), _DevBuf(cap), _DevBuf(8 * (B + 1)), _DevBuf(ws)
    try:
        d_in.upload(packed)
        d_fac.upload(fac)
        with pytest.raises(host.HipError) as e:                              # a workspace one byte too small
            host.flac_encode_ragged_device(d_in.ptr, lens, K.RATE, d_out.ptr, cap, d_off.ptr, d_ws.ptr, ws - 1, d_fac.ptr, 8000, lpc_order=lpc_order)
        assert e.value.code == host.E_INVALID
        host.flac_encode_ragged_device(d_in.ptr, lens, K.RATE, d_out.ptr, cap, d_off.ptr, d_ws.ptr, ws, d_fac.ptr, 8000, lpc_order=lpc_order)
        off = d_off.download((B + 1,), np.uint64)                            # (a blocking copy on the null stream: after the kernels)
        out = d_out.download((cap,), np.uint8)
    finally:
        for b in bufs:
            b.free()
    assert off.tolist() == want_off.tolist() and out[:int(off[-1])].tobytes() == want.tobytes()


@pytest.mark.parametrize("plan,seek", [(K.EXPORT, 8000), (K.UPLOAD, 0)])
@pytest.mark.parametrize("name", ["a", "d"])
def test_fused_entry_equals_normalize_then_encode(gpu, name, plan, seek):
    clips = K.burst(name)
    args = (plan["T"], plan["C"], plan["max_gain"], plan["gate_fallback"])
    res, streams = host.loudness_flac_ragged(clips, K.RATE, *args, seek, lpc_order=8)
    want_res, pcm = host.loudness_normalize_ragged(clips, K.RATE, *args)
    assert fields(res) == fields(want_res)
    assert streams == host.flac_encode_ragged(pcm, K.RATE, None, seek, lpc_order=8)
    for c, (s, y) in enumerate(zip(streams, pcm)):
        w = K.encode_one(y, seek, 8)
        assert s == w, (name, c, first_difference(s, w))


def test_surfaces_return_the_same_ragged_or_grouped(gpu):
    burst = list(K.burst("a"))
    kw = dict(max_gain_db=loudness.EXPORT_MAX_GAIN_DB, gate_fallback=True)
    ra, sa = flac.normalize_and_encode(burst, K.RATE, seek_interval=8000, lpc_order=8, ragged=True, **kw)
    rb, sb = flac.normalize_and_encode(burst, K.RATE, seek_interval=8000, lpc_order=8, ragged=False, **kw)
    assert fields(ra) == fields(rb) and sa == sb
    gains = [(-6.0, 0.0, 3.5)[c % 3] for c in range(len(burst))]
    assert flac.encode_clips(burst, K.RATE, gain_db=gains, lpc_order=4, ragged=True) == flac.encode_clips(burst, K.RATE, gain_db=gains, lpc_order=4)
    assert flac.encode_clips(burst, K.RATE, ragged=True) == flac.encode_clips(burst, K.RATE, ragged=False)
    for apply in (True, False):
        ra, oa = loudness.normalize_clips(burst, K.RATE, apply=apply, ragged=True, **kw)
        rb, ob = loudness.normalize_clips(burst, K.RATE, apply=apply, ragged=False, **kw)
        assert fields(ra) == fields(rb)
        assert (oa is None and ob is None) if not apply else all(np.array_equal(x, y) for x, y in zip(oa, ob))
