"""The device FLAC decoder (bnhip_flac_decode_*, bnhip_flac_spectrogram_png; flac.decode_clips, spectrogram.generate_from_flac) on the
GPU: the round trip of the project's own encoder, the feature streams of tests/flacmux.py against tests/flaclpcdec.py, a burst that
mixes valid and damaged streams, a CRC-valid frame image that is not on the chain, the fused decode + render + PNG entry byte for
byte against the PCM entry, and the device entry on a caller's stream and workspace."""
import ctypes as C
import os

import numpy as np
import pytest

import flaccases
import flacdeccases as K
import flaclpccases
import loudref
from birdnet_go_amd import flac, host, spectrogram as sg

from test_parity_gpu import _DevBuf

pytestmark = pytest.mark.gpu

STATUS = dict(OK=host.FLAC_OK, BAD_METADATA=host.FLAC_BAD_METADATA, UNSUPPORTED=host.FLAC_UNSUPPORTED, CORRUPT=host.FLAC_CORRUPT)


def _assert_decoded(clips, results, want, what=""):
    assert len(clips) == len(results) == len(want)
    for i, (c, r, x) in enumerate(zip(clips, results, want)):
        assert (r.status, r.fail_offset) == (host.FLAC_OK, 0), (what, i, r.status, r.frames, r.fail_offset)
        assert c is not None and c.dtype == np.int16 and c.size == x.size and np.array_equal(c, x), (what, i)


def _round_trip(cases, name):
    """encode_clips, then decode_clips: exactly the gained input.  (A case with factors goes through host.flac_encode, which
    encode_clips calls, since the cases state factors and encode_clips takes decibels; the expected samples are loudref.apply_gain of
    the input, with no Python decode.)"""
    case = cases.CASES[name]
    rate, clips, factor, seek = case[:4]
    lpc_order = case[4] if len(case) > 4 else 0
    if factor is None:
        want = [np.asarray(c, np.int16) for c in clips]
        streams = flac.encode_clips(list(clips), rate, seek_interval=seek, lpc_order=lpc_order)
    else:
        want = [loudref.apply_gain(c, float(factor[i])) for i, c in enumerate(clips)]
        streams = host.flac_encode(clips, rate, factor, seek, lpc_order=lpc_order)
    got, results = flac.decode_clips(streams)
    _assert_decoded(got, results, want, name)
    return results


@pytest.mark.parametrize("name", list(flaccases.CASES))
def test_round_trip_of_the_fixed_encoder(gpu, name):
    results = _round_trip(flaccases, name)
    if name == "two_byte_numbers":
        assert results[0].frames == 130
    if name == "three_byte_numbers":
        assert results[0].frames == 2050
    if name == "sixty_five":
        assert len(results) == 65


@pytest.mark.parametrize("name", list(flaclpccases.CASES))
def test_round_trip_of_the_lpc_encoder(gpu, name):
    _round_trip(flaclpccases, name)


def test_round_trip_of_ragged_lengths_in_one_call(gpu):
    lens = (1, 2, 3, 5, 16, 17, 255, 256, 257, 4095, 4096, 4097)
    clips = [np.ascontiguousarray(flaclpccases._mix(n, i)) for i, n in enumerate(lens)]
    streams = flac.encode_clips(clips, 48000, lpc_order=8, ragged=True, seek_interval=1000)
    got, results = flac.decode_clips(streams)
    _assert_decoded(got, results, clips)
    assert [r.frames for r in results] == [(n + 4095) // 4096 for n in lens]


def test_feature_streams_in_one_call_and_alone(gpu):
    streams = [K.feature(n)[0] for n in K.FEATURE_NAMES]
    want = [K.feature(n)[1] for n in K.FEATURE_NAMES]
    got, results = flac.decode_clips(streams)
    for i, n in enumerate(K.FEATURE_NAMES):
        _assert_decoded(got[i:i + 1], results[i:i + 1], want[i:i + 1], n)
        assert results[i].frames == len(K.feature(n)[2]["frames"]), n
    for n in ("bs16", "bs16384", "lpc32", "all_warmup"):                     # alone: the call's LDS follows its largest block size
        g, r = flac.decode_clips([K.feature(n)[0]])
        _assert_decoded(g, r, [K.feature(n)[1]], n)


def test_mixed_burst_of_valid_and_damaged_streams(gpu):
    _, _, intact, samples, info = K.three_frames()
    d = K.damaged()
    names = list(d)
    streams, kinds = [intact], ["valid"]
    for i, n in enumerate(names):
        streams += [d[n][0], K.feature(K.FEATURE_NAMES[i % len(K.FEATURE_NAMES)])[0] if i % 2 else intact]
        kinds += [n, "valid"]
    got, results = flac.decode_clips(streams)
    starts = [m["start"] for m in info["frames"]]
    for i, kind in enumerate(kinds):
        r = results[i]
        if kind == "valid":
            want = samples if streams[i] is intact else K.feature(K.FEATURE_NAMES[((i - 1) // 2) % len(K.FEATURE_NAMES)])[1]
            _assert_decoded(got[i:i + 1], results[i:i + 1], [want], f"neighbour {i}")
            continue
        _, status, fail = d[kind]
        assert got[i] is None, kind
        assert (r.status, r.fail_offset) == (STATUS[status], fail or 0), (kind, r.status, r.frames, r.fail_offset)
        if status == "UNSUPPORTED":
            assert r.frames == 0, kind
    by = dict(zip(kinds, results))
    assert by["crc16_flip"].frames == 1 and by["crc8_flip"].frames == 2 and by["truncated"].frames == 2
    assert by["trailing"].frames == 3 and by["missing_frame"].frames == 1 and by["overflow"].frames == 1
    assert starts[1] == d["crc16_flip"][2]


def test_a_valid_frame_image_off_the_chain_changes_nothing(gpu):
    s, want = K.off_chain()
    got, results = flac.decode_clips([s, s])
    _assert_decoded(got, results, [want, want])
    assert results[0].frames == 3


def _burst_clips(rate, lens, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(lens):
        t = np.arange(n)
        x = 9000.0 * np.sin(2.0 * np.pi * (700.0 + 900.0 * i) * t / rate) * (0.3 + 0.7 * np.sin(2.0 * np.pi * 3.0 * t / rate) ** 2)
        out.append(np.clip(np.round(x + rng.normal(0.0, 300.0, n)), -32768, 32767).astype(np.int16))
    return out


LENS = (30000, 48000, 4097, 12345, 70001)


@pytest.mark.parametrize("rate_out", [24000, 0])
def test_fused_entry_equals_the_pcm_entry_byte_for_byte(gpu, rate_out):
    clips = _burst_clips(48000, LENS, 5)
    streams = flac.encode_clips(clips, 48000, lpc_order=8, ragged=True, seek_interval=48000)
    kw = sg._render_args(48000, 258, sg.bird_profile(), "default", "100")
    assert kw["rate_out"] == 24000
    kw["rate_out"] = rate_out
    pal = sg.palette("default")
    want = host.spectrogram_png_ragged(clips, 48000, 258, pal, **kw)
    got, results = host.flac_spectrogram_png(streams, 258, pal, **kw)
    assert [(r.status, r.fail_offset) for r in results] == [(host.FLAC_OK, 0)] * len(clips)
    assert [r.frames for r in results] == [(n + 4095) // 4096 for n in LENS]
    assert got == want


def test_generate_from_flac_groups_by_rate(gpu, tmp_path):
    a, b = _burst_clips(48000, (30000, 9000), 6), _burst_clips(32000, (20000, 5000, 8193), 7)
    sa, sb = flac.encode_clips(a, 48000, lpc_order=8, ragged=True), flac.encode_clips(b, 32000, lpc_order=4, ragged=True)
    corrupt = bytearray(sa[0])
    corrupt[len(corrupt) // 2] ^= 0x40
    streams = [sa[0], sb[0], sb[1], sa[1], bytes(corrupt), sb[2], K.damaged()["stereo"][0]]
    paths = [str(tmp_path / f"f{i}.png") for i in range(len(streams))]
    status = sg.generate_from_flac(streams, paths, 258)
    assert status == [host.FLAC_OK] * 4 + [host.FLAC_CORRUPT, host.FLAC_OK, host.FLAC_UNSUPPORTED]
    assert not os.path.exists(paths[4]) and not os.path.exists(paths[6])
    wa = [str(tmp_path / f"a{i}.png") for i in range(2)]
    wb = [str(tmp_path / f"b{i}.png") for i in range(3)]
    sg.generate_burst(a, wa, 258, 48000, device_png=True, ragged=True)
    sg.generate_burst(b, wb, 258, 32000, device_png=True, ragged=True)
    read = lambda p: open(p, "rb").read()
    # (a burst's PNG streams do not depend on their neighbours: the corrupt stream in the 48 kHz call changes no other file)
    assert [read(paths[i]) for i in (0, 3)] == [read(p) for p in wa]
    assert [read(paths[i]) for i in (1, 2, 5)] == [read(p) for p in wb]


def test_device_entry_on_a_caller_stream_and_workspace(gpu):
    names = ("bs576", "lpc32", "escapes", "last16")
    streams = [K.feature(n)[0] for n in names] + [K.damaged()["crc16_flip"][0], K.damaged()["bits24"][0]]
    want = [K.feature(n)[1] for n in names]
    host_clips, host_results = host.flac_decode(streams)
    buf, offsets = host._flac_burst(streams)
    infos = [flac.stream_info(s) for s in streams]
    total = sum(int(i.total_samples) for i in infos if i.status == host.FLAC_OK)
    ws = host.flac_decode_workspace_size(infos, offsets)
    n = len(streams)
    bufs = d_in, d_pcm, d_res, d_ws = _DevBuf(buf.nbytes), _DevBuf(2 * total), _DevBuf(16 * n), _DevBuf(ws)
    hip = _DevBuf._hip
    stream = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    try:
        d_in.upload(buf)
        with pytest.raises(host.HipError) as e:                              # a workspace one byte too small
            host.flac_decode_device(d_in.ptr, offsets, infos, d_pcm.ptr, total, d_res.ptr, d_ws.ptr, ws - 1, hip_stream_ptr=stream)
        assert e.value.code == host.E_INVALID
        host.flac_decode_device(d_in.ptr, offsets, infos, d_pcm.ptr, total, d_res.ptr, d_ws.ptr, ws, hip_stream_ptr=stream)
        assert hip.hipStreamSynchronize(stream) == 0
        pcm = d_pcm.download((total,), np.int16)
        res = d_res.download((n, 4), np.int32)
    finally:
        hip.hipStreamDestroy(stream)
        for b in bufs:
            b.free()
    lens = [int(i.total_samples) if i.status == host.FLAC_OK else 0 for i in infos]
    clips = host.ragged_unpack(pcm, lens)
    for i in range(len(names)):
        assert np.array_equal(clips[i], want[i]) and np.array_equal(host_clips[i], want[i]), names[i]
    fail = res[:, 2].astype(np.uint32).astype(np.uint64) | (res[:, 3].astype(np.uint32).astype(np.uint64) << np.uint64(32))
    assert [(int(res[i, 0]), int(res[i, 1]), int(fail[i])) for i in range(n)] == [(r.status, r.frames, r.fail_offset) for r in host_results]
    assert [r.status for r in host_results] == [host.FLAC_OK] * 4 + [host.FLAC_CORRUPT, host.FLAC_UNSUPPORTED]
