"""The FLAC decode entries without a device (bnhip_flac_stream_info, bnhip_flac_decode_*, bnhip_flac_spectrogram_png): the symbols and
their declarations, bnhip_flac_stream_info against tests/flaclpcdec.read_metadata on the encoder's streams, on streams with further
metadata blocks, on every rejection and on every truncation of a 42-byte head, and the argument errors answered before any device is
touched."""
import ctypes as C
import os

import numpy as np
import pytest

import flaccases
import flacdeccases as K
import flaclpccases
import flaclpcdec
import flacmux
from birdnet_go_amd import flac, host

ENTRIES = ("bnhip_flac_stream_info", "bnhip_flac_decode_workspace_size", "bnhip_flac_decode_device", "bnhip_flac_decode_pcm16",
           "bnhip_flac_spectrogram_png")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bnhip.h")
FIELDS = ("rate", "bits", "channels", "min_block", "max_block", "min_frame", "max_frame")


def test_symbols_are_exported_and_declared(built_lib):
    lib = C.CDLL(built_lib)
    with open(HEADER) as fh:
        header = fh.read()
    for s in ENTRIES:
        assert s in host.SYMBOLS and hasattr(lib, s), s
        assert f"int {s}(" in header, s
    assert "NOT verified" in header                       # the MD5


def _split(blob, offsets):
    return [blob[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]


def _check_against_read_metadata(stream):
    info = flac.stream_info(stream)
    want, seek, audio = flaclpcdec.read_metadata(bytes(stream))
    assert info.status == host.FLAC_OK
    assert {f: getattr(info, f) for f in FIELDS} == {f: want[f] for f in FIELDS}
    assert (info.total_samples, info.audio_offset, info.seek_points) == (want["total"], audio, len(seek))


@pytest.mark.parametrize("name", ["contents_one_clip", "len1", "len17", "len4097", "rate256000", "rate11025", "two_byte_numbers"])
def test_stream_info_on_the_encoder_streams(built_lib, name):
    blob, offsets, _, _ = flaccases.reference(name)
    for s in _split(blob, offsets):
        _check_against_read_metadata(s)


@pytest.mark.parametrize("name", ["contents_one_clip", "len5", "len8225", "contents_order1"])
def test_stream_info_on_the_lpc_streams(built_lib, name):
    blob, offsets, _, _ = flaclpccases.reference(name)
    for s in _split(blob, offsets):
        _check_against_read_metadata(s)


@pytest.mark.parametrize("name", K.FEATURE_NAMES)
def test_stream_info_on_the_feature_streams(built_lib, name):
    _check_against_read_metadata(K.feature(name)[0])


def test_stream_info_rejections(built_lib):
    x = np.arange(-300, 300)
    good = flacmux.stream(x, 192, 48000)
    si = flacmux.streaminfo(192, 48000, 600, 20, 400)
    frames = good[42:]
    BAD, UNS = host.FLAC_BAD_METADATA, host.FLAC_UNSUPPORTED

    def status(s):
        info = flac.stream_info(s)
        return info.status

    assert status(good) == host.FLAC_OK
    cases = {
        "no marker": (b"fLaX" + good[4:], BAD),
        "empty": (b"", BAD),
        "marker only": (b"fLaC", BAD),
        "STREAMINFO not first": (b"fLaC" + flacmux.block(1, bytes(8)) + flacmux.block(0, si, last=True) + frames, BAD),
        "STREAMINFO repeated": (b"fLaC" + flacmux.block(0, si) + flacmux.block(0, si, last=True) + frames, BAD),
        "STREAMINFO of 33 bytes": (b"fLaC" + flacmux.block(0, si[:33], last=True) + frames, BAD),
        "STREAMINFO of 35 bytes": (b"fLaC" + flacmux.block(0, si + b"\0", last=True) + frames, BAD),
        "truncated block": (b"fLaC" + flacmux.block(0, si) + flacmux.block(1, bytes(100), last=True)[:50], BAD),
        "truncated block header": (b"fLaC" + flacmux.block(0, si) + b"\x81\0", BAD),
        "no last block": (b"fLaC" + flacmux.block(0, si), BAD),
        "block type 127": (b"fLaC" + flacmux.block(0, si) + flacmux.block(127, bytes(4), last=True) + frames, BAD),
        "min block 15": (flacmux.stream(x, 192, 48000, info=dict(min_block=15)), BAD),
        "bounds inverted": (flacmux.stream(x, 192, 48000, info=dict(min_block=193)), BAD),
        "stereo": (flacmux.stream(x, 192, 48000, info=dict(channels=2)), UNS),
        "8 bits": (flacmux.stream(x, 192, 48000, info=dict(bits=8)), UNS),
        "24 bits": (flacmux.stream(x, 192, 48000, info=dict(bits=24)), UNS),
        "variable block size": (flacmux.stream(x, 192, 48000, dict(kind="FIXED", order=1, variable=True)), UNS),
        "total 0": (flacmux.stream(x, 192, 48000, info=dict(total=0)), UNS),
        "total 2^31": (flacmux.stream(x, 192, 48000, info=dict(total=1 << 31)), UNS),
        "min != max, several frames": (flacmux.stream(x, 192, 48000, info=dict(min_block=16)), UNS),
        "block size 32768": (flacmux.stream(x, 192, 48000, info=dict(bs=32768, min_block=32768)), UNS),
    }
    for what, (s, want) in cases.items():
        assert status(s) == want, what
        if want == BAD:
            with pytest.raises(flaclpcdec.FlacError):
                flaclpcdec.read_metadata(s)
    # min != max with a single frame is a stream like any other; 2^31 - 1 samples is the largest count
    assert status(flacmux.stream(x[:100], 192, 48000, info=dict(min_block=16))) == host.FLAC_OK
    assert status(flacmux.stream(x, 192, 48000, info=dict(total=(1 << 31) - 1))) == host.FLAC_OK


def test_stream_info_on_every_truncation_of_a_head(built_lib):
    s = flacmux.stream(np.arange(40), 192, 48000)
    assert len(s) > 42 and flac.stream_info(s[:42]).status == host.FLAC_OK          # (the frames are the device's business)
    for cut in range(42):
        assert flac.stream_info(s[:cut]).status == host.FLAC_BAD_METADATA, cut


def test_errors_before_any_device(built_lib):
    lib = host.load_library()
    ci, vp, sz, cd = C.c_int, C.c_void_p, C.c_size_t, C.c_double
    err = lambda: lib.bnhip_last_error()
    lib.bnhip_last_error.restype = C.c_char_p
    streams = [K.feature("bs192")[0], K.feature("lpc1")[0]]
    buf, offsets = host._flac_burst(streams)
    infos = (host.FlacInfo * 2)(*[flac.stream_info(s) for s in streams])
    total = sum(int(i.total_samples) for i in infos)
    pcm, lens, res = np.zeros(total, np.int16), np.zeros(2, np.int32), (host.FlacDecodeResult * 2)()
    W, H = 258, 129
    cap0 = host.png_max_bytes(2, W, H)
    outb, pal, poff = np.zeros(cap0, np.uint8), np.zeros(768, np.uint8), np.zeros(3, np.uint64)
    need = host.flac_decode_workspace_size(list(infos), offsets)
    assert need > 0 and need % 256 == 0
    wsb = np.zeros(need + 512, np.uint8)
    aligned = (wsb.ctypes.data + 255) & ~255
    dev = ci(99)                                                             # no such device: a valid call fails differently, later
    b = sz(0)

    def run(which, n=2, off=offsets, inf=infos, data=vp(buf.ctypes.data), cap=total, ws=need, wsp=aligned, out_cap=cap0, rate_out=24000,
            width=W, height=H, results=vp(C.addressof(res))):
        O = vp(off.ctypes.data) if off is not None else vp()
        I = vp(C.addressof(inf)) if inf is not None else vp()
        if which == "info":
            return lib.bnhip_flac_stream_info(data, sz(10), I)
        if which == "ws":
            return lib.bnhip_flac_decode_workspace_size(ci(n), I, O, C.byref(b))
        if which == "device":
            return lib.bnhip_flac_decode_device(dev, data, ci(n), O, I, vp(pcm.ctypes.data), sz(cap), results, vp(wsp), sz(ws), vp())
        if which == "pcm16":
            return lib.bnhip_flac_decode_pcm16(dev, data, ci(n), O, vp(pcm.ctypes.data), sz(cap), vp(lens.ctypes.data), results)
        return lib.bnhip_flac_spectrogram_png(dev, data, ci(n), O, ci(rate_out), ci(width), ci(height), vp(), cd(0.0), cd(100.0),
                                              vp(pal.ctypes.data), vp(outb.ctypes.data), sz(out_cap), vp(poff.ctypes.data), results)

    assert run("info", data=vp()) == host.E_INVALID and err() == b"NULL/empty argument"
    assert run("info", inf=None) == host.E_INVALID and err() == b"NULL/empty argument"
    for w in ("ws", "device", "pcm16", "png"):
        assert run(w, off=None) == host.E_INVALID and err() == b"NULL/empty argument", w
        assert run(w, n=0) == host.E_INVALID and b"n_streams" in err(), w
        assert run(w, n=65536) == host.E_INVALID and b"n_streams" in err(), w
        assert run(w, off=np.array([0, 500, 400], np.uint64)) == host.E_INVALID and b"ascend" in err(), w
    for w in ("device", "pcm16", "png"):
        assert run(w, data=vp()) == host.E_INVALID and err() == b"NULL/empty argument", w
        assert run(w, results=vp()) == host.E_INVALID and err() == b"NULL/empty argument", w
    assert run("ws", inf=None) == host.E_INVALID and err() == b"NULL/empty argument"
    for w in ("device", "pcm16"):
        assert run(w, cap=total - 1) == host.E_INVALID and b"pcm_cap_samples" in err(), w
    assert run("device", ws=need - 1) == host.E_INVALID and b"workspace" in err()
    assert run("device", wsp=aligned + 128) == host.E_INVALID and b"aligned" in err()
    assert run("device", wsp=0) == host.E_INVALID and err() == b"NULL/empty argument"
    lying = (host.FlacInfo * 2)(*infos)
    lying[1].audio_offset = len(streams[1]) + 1
    assert run("device", inf=lying) == host.E_INVALID and b"BNHIP_FLAC_OK" in err()
    lying[1].audio_offset = infos[1].audio_offset
    lying[1].max_block = 32768
    assert run("ws", inf=lying) == host.E_INVALID and b"BNHIP_FLAC_OK" in err()
    same_buf, same_off = host._flac_burst([streams[0], streams[0]])
    same = dict(data=vp(same_buf.ctypes.data), off=same_off)
    assert run("png", out_cap=cap0 - 1, **same) == host.E_INVALID and b"out_cap" in err()
    assert run("png", width=0, **same) == host.E_INVALID and b"width" in err()
    assert run("png", height=130, **same) == host.E_INVALID and b"height" in err()
    assert run("png", rate_out=-1, **same) == host.E_INVALID and b"sample rates" in err()
    # the fused entry wants accepted metadata and one rate (48000 and 32000 here)
    assert run("png") == host.E_INVALID and b"same sample rate" in err()
    bad_buf, bad_off = host._flac_burst([streams[0], K.damaged()["stereo"][0]])
    assert run("png", data=vp(bad_buf.ctypes.data), off=bad_off) == host.E_INVALID and b"metadata" in err()
    # valid calls get as far as the device ordinal
    for w in ("device", "pcm16"):
        rc = run(w)
        assert rc != host.BNHIP_OK and (rc != host.E_INVALID or b"device ordinal" in err()), w
    rc = run("png", **same)
    assert rc != host.BNHIP_OK and (rc != host.E_INVALID or b"device ordinal" in err())
    assert run("ws") == host.BNHIP_OK and b.value == need


def test_python_surface_without_a_device(built_lib):
    info = flac.stream_info(K.feature("rate13")[0])
    assert (info.rate, info.bits, info.channels, info.status) == (11025, 16, 1, host.FLAC_OK)
    with pytest.raises(host.HipError):
        host._flac_burst([])
