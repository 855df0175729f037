"""The recording decoder on the GPU (bnhip_flac_recording_info, bnhip_flac_decode_recordings*, flac.decode_recordings): stereo and
24-bit FLAC streams to interleaved PCM at their own depth.  The criterion is byte equality with tests/flacwidedec.py, the decoder
restatement, on the streams of tests/flacwidecases.py (whose muxer / restatement round trip and whose pass through flac_parse.h
under the sanitizers are tests/test_flac_wide_ref.py): the four stereo assignments at both depths, the extremes that need the side
channel's extra bit, wasted bits that differ between the subframes, every subframe kind in both channels, the 24-bit LPC sums that
do not fit 32-bit products, block sizes with short last frames, the wide cap and the mono cap, a burst packed at odd bytes between
guard bytes, and the damaged streams."""
import ctypes as C

import numpy as np
import pytest

import flacwidecases as K
import flacwidedec as D
from birdnet_go_amd import flac, host

from test_parity_gpu import _DevBuf

pytestmark = pytest.mark.gpu

STATUS = dict(OK=host.FLAC_OK, BAD_METADATA=host.FLAC_BAD_METADATA, UNSUPPORTED=host.FLAC_UNSUPPORTED, CORRUPT=host.FLAC_CORRUPT)


@pytest.fixture(scope="module")
def decoded(gpu):
    """Every case in one call: name -> (its PCM bytes, its result)."""
    names = list(K.cases())
    pcm, offsets, results = host.flac_decode_recordings([K.cases()[n][0] for n in names], guard=64)
    return {n: (pcm[int(offsets[i]):int(offsets[i + 1])].tobytes(), results[i]) for i, n in enumerate(names)}


@pytest.mark.parametrize("name", list(K.cases()))
def test_every_case_decodes_to_the_restatement_bytes(decoded, name):
    s, x, bits = K.cases()[name]
    pcm, r = decoded[name]
    assert (r.status, r.fail_offset) == (host.FLAC_OK, 0), (r.status, r.frames, r.fail_offset)
    assert r.frames == -(-x.shape[0] // host.flac_recording_info(s).max_block)
    assert pcm == D.pcm_bytes(x, bits)


@pytest.mark.parametrize("name", ["lpc32_overflow_24", "cap_8192_24", "mono16_16384", "bs16_49_24", "extremes_mid_side_24", "mono_16"])
def test_a_case_alone_sizes_the_launch_by_its_own_frames(gpu, name):
    s, x, bits = K.cases()[name]
    got, results = flac.decode_recordings([s])
    assert results[0].status == host.FLAC_OK
    assert got[0].dtype == (np.int16 if bits == 16 else np.int32) and got[0].shape == x.shape and np.array_equal(got[0], x)
    assert flac.decode_recordings([s], as_bytes=True)[0][0] == D.pcm_bytes(x, bits)


def test_a_stream_above_the_wide_cap_is_refused_by_the_info_entry(gpu):
    s = K.above_cap()
    assert flac.recording_info(s).status == host.FLAC_UNSUPPORTED
    ok = K.cases()["mono_24"]
    got, results = flac.decode_recordings([s, ok[0]])
    assert got[0] is None and (results[0].status, results[0].frames, results[0].fail_offset) == (host.FLAC_UNSUPPORTED, 0, 0)
    assert np.array_equal(got[1], ok[1]) and results[1].status == host.FLAC_OK
    # an info marked OK by hand does not get a stream past the check
    info = flac.recording_info(s)
    info.status = host.FLAC_OK
    with pytest.raises(host.HipError) as e:
        host.flac_decode_recordings_workspace_size([info], [0, len(s)])
    assert e.value.code == host.E_INVALID and "bnhip_flac_recording_info" in str(e.value)


def test_a_packed_burst_starts_recordings_at_odd_bytes_between_untouched_guards(gpu):
    burst = K.packing()
    pcm, offsets, results = host.flac_decode_recordings([s for s, _, _ in burst], guard=256)      # (raises if a guard byte changed)
    want = [D.pcm_bytes(x, bits) for _, x, bits in burst]
    assert [int(o) for o in offsets] == list(np.cumsum([0] + [len(w) for w in want]))
    assert [int(o) % 2 for o in offsets[:4]] == [0, 1, 1, 1] and len(want[0]) == 15
    assert [r.status for r in results] == [host.FLAC_OK] * 5
    assert pcm.tobytes() == b"".join(want)
    for order in ((4, 2, 0, 1, 3), (2, 3, 4, 0, 1)):          # other alignments of the same recordings
        p, o, r = host.flac_decode_recordings([burst[i][0] for i in order], guard=256)
        assert p.tobytes() == b"".join(want[i] for i in order) and [q.status for q in r] == [host.FLAC_OK] * 5


def test_damaged_recordings_keep_what_lies_in_front_of_the_damage(gpu):
    d = K.damaged()
    names = list(d)
    intact = K.cases()["side_right_24"]
    streams = []
    for n in names:
        streams += [d[n][0], intact[0]]
    got, results = flac.decode_recordings(streams, as_bytes=True)
    for i, n in enumerate(names):
        _, status, frames, fail, kept, bits = d[n]
        r = results[2 * i]
        assert (r.status, r.frames, r.fail_offset) == (STATUS[status], frames, fail), n
        assert got[2 * i] == D.pcm_bytes(kept, bits), n
        assert results[2 * i + 1].status == host.FLAC_OK and got[2 * i + 1] == D.pcm_bytes(intact[1], intact[2]), n


def test_the_clip_entries_answer_stereo_and_24_bit_streams_as_before(gpu):
    s24, s16 = K.cases()["mid_side_24"][0], K.cases()["left_side_16"][0]
    mono = K.cases()["mono_16"]
    clips, results = flac.decode_clips([s24, mono[0], s16])
    assert [r.status for r in results] == [host.FLAC_UNSUPPORTED, host.FLAC_OK, host.FLAC_UNSUPPORTED]
    assert clips[0] is None and clips[2] is None and np.array_equal(clips[1], mono[1][:, 0])


def test_device_entry_on_a_caller_stream_and_workspace(gpu):
    names = ("mid_side_24", "wasted_side_16", "mono_24", "lpc32_overflow_24")
    streams = [K.cases()[n][0] for n in names] + [K.damaged()["range_24"][0], K.above_cap()]
    want = [D.pcm_bytes(K.cases()[n][1], K.cases()[n][2]) for n in names] + [D.pcm_bytes(K.damaged()["range_24"][4], 24), b""]
    buf, offsets = host._flac_burst(streams)
    infos = [flac.recording_info(s) for s in streams]
    total = sum(len(w) for w in want)
    ws = host.flac_decode_recordings_workspace_size(infos, offsets)
    n = len(streams)
    bufs = d_in, d_pcm, d_res, d_ws = _DevBuf(buf.nbytes), _DevBuf(total + 8), _DevBuf(16 * n), _DevBuf(ws)
    hip = _DevBuf._hip
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        d_in.upload(buf)
        d_pcm.upload(np.full(total + 8, 0x5A, np.uint8))
        with pytest.raises(host.HipError) as e:
            host.flac_decode_recordings_device(d_in.ptr, offsets, infos, d_pcm.ptr, total - 1, d_res.ptr, d_ws.ptr, ws, hip_stream_ptr=stream)
        assert e.value.code == host.E_INVALID
        host.flac_decode_recordings_device(d_in.ptr, offsets, infos, d_pcm.ptr, total, d_res.ptr, d_ws.ptr, ws, hip_stream_ptr=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        pcm = d_pcm.download((total + 8,), np.uint8)
        res = d_res.download((n, 4), np.int32)
    finally:
        hip.hipStreamDestroy(stream)
        for b in bufs:
            b.free()
    assert pcm[:total].tobytes() == b"".join(want) and np.all(pcm[total:] == 0x5A)
    assert [int(v) for v in res[:, 0]] == [host.FLAC_OK] * 4 + [host.FLAC_CORRUPT, host.FLAC_UNSUPPORTED]
