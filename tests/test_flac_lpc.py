"""The LPC predictors of the FLAC encoder on the device (bnhip_flac_lpc_*, bnhip_loudness_flac_lpc_pcm16) against the restatement of
the spec (tests/flaclpcref.py) and an independent decoder (tests/flaclpcdec.py).

Acceptance: the autocorrelation is integer arithmetic and the recursion fp64 with one rounding per operation in the spec's order, so
every byte and every offset equals the restatement's; lpc_order 0 is the encoder without LPC byte for byte; the device entry equals
the host entry; the fused entry equals bnhip_loudness_normalize_pcm16 followed by the encode, records and bytes; the owl recording
shrinks.  The cases (tests/flaclpccases.py) run as batches of 1, 3 and 65 clips at lpc_order 1, 4 and 8."""
import ctypes as C
import os

import numpy as np
import pytest

import flaccases
import flaclpccases as K
import flaclpcdec
import flaclpcref
from birdnet_go_amd import flac, host

from test_flac import EXPORT, UPLOAD, fields, first_difference, loud_batch
from test_parity_gpu import _DevBuf

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name", list(K.CASES))
def test_bytes_and_offsets_equal_the_restatement(gpu, name):
    rate, clips, factor, seek, M = K.CASES[name]
    want, want_off, _, gained = K.reference(name)
    got, off = host.flac_encode(clips, rate, factor, seek, raw=True, lpc_order=M)
    assert off.tolist() == want_off.tolist(), name
    assert got.tobytes() == want, (name, first_difference(got.tobytes(), want))
    assert int(off[-1]) <= host.flac_max_bytes(len(clips), clips.shape[1], seek)
    for c in range(min(len(clips), 2)):                                  # (the restatement's own streams decode in test_flac_lpc_ref.py)
        y, info = flaclpcdec.decode(got[int(off[c]):int(off[c + 1])].tobytes())
        assert np.array_equal(y, gained[c]) and info["rate"] == rate, (name, c)


@pytest.mark.parametrize("name", ["contents_one_clip", "sixty_five"])
def test_order_zero_is_the_encoder_without_lpc(gpu, name):
    """Through the new entry with 0, through the entry of before, and the restatement without LPC: the same bytes."""
    rate, clips, factor, seek = flaccases.CASES[name]
    want, want_off, _, _ = flaccases.reference(name)
    got, off = host.flac_encode(clips, rate, factor, seek, raw=True, lpc_order=0)
    plain, plain_off = host.flac_encode(clips, rate, factor, seek, raw=True)
    assert off.tolist() == plain_off.tolist() == want_off.tolist() and got.tobytes() == plain.tobytes() == want
    lib = host.load_library()
    Bc, n = clips.shape
    x = np.ascontiguousarray(clips)
    fac = None if factor is None else np.ascontiguousarray(factor, np.float64)
    cap = host.flac_max_bytes(Bc, n, seek)
    out, old_off = np.empty(cap, np.uint8), np.zeros(Bc + 1, np.uint64)
    lib.bnhip_flac_encode_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    assert lib.bnhip_flac_encode_pcm16(0, x.ctypes.data, Bc, n, rate, fac.ctypes.data if fac is not None else None, seek, out.ctypes.data, cap,
                                       old_off.ctypes.data) == host.BNHIP_OK
    assert old_off.tolist() == want_off.tolist() and out[:int(old_off[-1])].tobytes() == want


@pytest.mark.parametrize("name", ["contents_one_clip", "len257", "len8225", "sixty_five"])
def test_device_entry_equals_the_host_entry(gpu, name):
    rate, clips, factor, seek, M = K.CASES[name]
    Bc, n = clips.shape
    want, want_off = host.flac_encode(clips, rate, factor, seek, raw=True, lpc_order=M)
    cap, ws = host.flac_max_bytes(Bc, n, seek), host.flac_lpc_workspace_size(Bc, n, M)
    bufs = d_in, d_fac, d_out, d_off, d_ws = _DevBuf(clips.nbytes), _DevBuf(8 * Bc), _DevBuf(cap), _DevBuf(8 * (Bc + 1)), _DevBuf(ws)
    try:
        d_in.upload(np.ascontiguousarray(clips))
        if factor is not None:
            d_fac.upload(np.ascontiguousarray(factor, np.float64))
        host.flac_encode_device(d_in.ptr, Bc, n, rate, d_out.ptr, cap, d_off.ptr, d_ws.ptr, ws, d_fac.ptr if factor is not None else None, seek,
                                lpc_order=M)
        off = d_off.download((Bc + 1,), np.uint64)                       # (a blocking copy on the null stream: after the kernels)
        out = d_out.download((cap,), np.uint8)
        with pytest.raises(host.HipError) as e:                          # the workspace of the encoder without LPC is too small
            host.flac_encode_device(d_in.ptr, Bc, n, rate, d_out.ptr, cap, d_off.ptr, d_ws.ptr, host.flac_workspace_size(Bc, n), None, seek,
                                    lpc_order=M)
        assert e.value.code == host.E_INVALID
    finally:
        for b in bufs:
            b.free()
    assert off.tolist() == want_off.tolist() and out[:int(off[-1])].tobytes() == want.tobytes()


@pytest.mark.parametrize("rate,n,count,plan,seek", [(8000, 5 * 800 + 37, 5, EXPORT, 8000), (8000, 5 * 800 + 37, 5, UPLOAD, 0)])
def test_fused_entry_equals_normalize_then_encode(gpu, rate, n, count, plan, seek):
    clips = loud_batch(rate, n, count)
    res, streams = host.loudness_flac(clips, rate, plan["T"], plan["C"], plan["max_gain"], plan["gate_fallback"], seek, lpc_order=8)
    want_res, pcm = host.loudness_normalize(clips, rate, plan["T"], plan["C"], plan["max_gain"], plan["gate_fallback"])
    assert fields(res) == fields(want_res)
    assert any(g.gain_db != 0.0 for g in res)
    assert streams == host.flac_encode(pcm, rate, None, seek, lpc_order=8)
    assert streams == [flaclpcref.encode(y, rate, seek, 8) for y in pcm]
    for s, y in zip(streams, pcm):
        assert np.array_equal(flaclpcdec.decode(s)[0], y)
    burst = [clips[0], clips[1][:4 * 800], clips[2]]
    r2, s2 = flac.normalize_and_encode(burst, rate, max_gain_db=plan["max_gain"], gate_fallback=plan["gate_fallback"], seek_interval=seek,
                                       lpc_order=flac.LEVEL5_LPC_ORDER)
    assert s2[0] == streams[0] and s2[2] == streams[2] and fields(r2)[0] == fields(res)[0]
    assert flac.encode_clips(burst, rate, lpc_order=4)[1] == flaclpcref.encode(burst[1], rate, 0, 4)


def test_tawny_owl_is_identical_to_the_restatement_and_smaller_than_without_lpc(gpu):
    """The reference's own recording (48 kHz, five 3 s clips), reduced to 16 bits: the first 40 frames."""
    pcm = K.owl_pcm16(GOLDEN)
    got = host.flac_encode(pcm, 48000, lpc_order=8)[0]
    assert got == flaclpcref.encode(pcm, 48000, 0, 8)
    without = host.flac_encode(pcm, 48000)[0]
    print(f"tawny owl, 40 frames at 16 bits: {len(got)} bytes with LPC orders 1..8, {len(got) / (2.0 * pcm.size):.4f} of the PCM; "
          f"{len(without)} bytes, {len(without) / (2.0 * pcm.size):.4f}, without")
    assert len(got) < len(without)


def test_lpc_order_outside_the_range_is_invalid(gpu):
    x = np.zeros((2, 1000), np.int16)
    for bad in (9, -1):
        for call in (lambda: host.flac_encode(x, 48000, lpc_order=bad), lambda: host.loudness_flac(x, 48000, lpc_order=bad),
                     lambda: host.flac_lpc_workspace_size(2, 1000, bad),
                     lambda: host.flac_encode_device(1 << 20, 2, 1000, 48000, 1 << 20, 1 << 20, 1 << 20, 1 << 20, 1 << 20, lpc_order=bad)):
            with pytest.raises(host.HipError) as e:
                call()
            assert e.value.code == host.E_INVALID and "lpc_order" in str(e.value)
