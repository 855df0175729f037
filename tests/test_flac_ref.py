"""FLAC on the CPU: the restatement of the encoder spec (tests/flacref.py) against an independent decoder written from RFC 9639
(tests/flacdec.py), the branches the shared cases (tests/flaccases.py) reach, the decoder's rejections, and the C ABI's argument
errors (answered before any device is touched)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import birdnet_go_amd  # noqa: F401
from birdnet_go_amd import flac, host

import flaccases as K
import flacdec
import flacref

INF = math.inf
ENTRIES = ("bnhip_flac_max_bytes", "bnhip_flac_workspace_size", "bnhip_flac_encode_device", "bnhip_flac_encode_pcm16", "bnhip_loudness_flac_pcm16")


def test_crc_check_values():
    """CRC-8/SMBUS and CRC-16/UMTS of the catalogue's check string, by both implementations."""
    assert flacref.crc8(b"123456789") == 0xF4 and flacref.crc16(b"123456789") == 0xFEE8
    assert flacdec.crc8(b"123456789") == 0xF4 and flacdec.crc16(b"123456789") == 0xFEE8
    rng = np.random.default_rng(0)
    for n in (0, 1, 2, 255, 8211):
        d = rng.integers(0, 256, n).astype(np.uint8).tobytes()
        assert flacref.crc16(d) == flacdec.crc16(d) and flacref.crc8(d) == flacdec.crc8(d)


def test_coded_numbers_of_every_length():
    for v, nb in [(0, 1), (127, 1), (128, 2), (2047, 2), (2048, 3), (65535, 3), (65536, 4), (2**21 - 1, 4), (2**21, 5), (2**26 - 1, 5),
                  (2**26, 6), (2**31 - 1, 6), (2**31, 7), (2**36 - 1, 7)]:
        b = flacref.coded_number(v)
        assert len(b) == nb and flacdec.read_coded_number(b, 0) == (v, nb), v


@pytest.mark.parametrize("name", list(K.CONTENTS))
def test_each_content_reaches_its_branch(name):
    want = K.CONTENTS[name][1]
    s, info = flacref.encode(K.content(name), 48000, info=True)
    f = info[0]
    assert f["kind"] == want[0], (name, f)
    if want[0] == "FIXED":
        _, o, P, k = want
        assert (o is None or f["order"] == o) and (P is None or f["porder"] == P) and (k is None or k in f["ks"]), (name, f)
    y, _ = flacdec.decode(s)
    assert np.array_equal(y, K.content(name))


@pytest.mark.parametrize("name", list(K.CASES))
def test_decoder_returns_the_input_of_the_restatement(built_lib, name):
    rate, clips, _, seek = K.CASES[name]
    buf, off, infos, gained = K.reference(name)
    assert int(off[-1]) <= host.flac_max_bytes(len(clips), clips.shape[1], seek)
    for c, g in enumerate(gained):
        s = buf[int(off[c]):int(off[c + 1])]
        assert len(s) <= host.flac_max_bytes(1, g.size, seek)
        y, info = flacdec.decode(s)
        assert np.array_equal(y, g), (name, c)
        assert info["rate"] == rate and info["bits"] == 16 and info["total"] == g.size and info["md5"] == bytes(16)
        assert (info["min_block"], info["max_block"]) == (4096, 4096)
        assert len(info["seek"]) == len(flacref.seek_frames(g.size, seek))
        for m, r in zip(info["frames"], infos[c]):                        # the decoder reads back what the encoder chose
            assert m["kind"] == r["kind"] and m["bs"] == r["bs"] and m["bytes"] == r["bytes"] and m["wasted"] == 0
            if r["kind"] == "FIXED":
                assert (m["order"], m["porder"], m["ks"], m["method"]) == (r["order"], r["porder"], r["ks"], 0)


def test_the_cases_reach_every_branch():
    frames = [f for name in K.CASES for clip in K.reference(name)[2] for f in clip]
    fixed = [f for f in frames if f["kind"] == "FIXED"]
    assert {f["kind"] for f in frames} == {"CONSTANT", "VERBATIM", "FIXED"}
    assert {f["order"] for f in fixed} == {0, 1, 2, 3, 4}
    assert {f["porder"] for f in fixed} == {0, 1, 2, 3, 4, 5}
    ks = {k for f in fixed for k in f["ks"]}
    assert 0 in ks and 14 in ks and max(ks) <= 14
    assert {f["number_bytes"] for f in frames} == {1, 2, 3}
    assert {f["bs_code"] for f in frames} == {12, 6, 7}
    codes = {f["rate_code"] for f in frames}
    assert 0 in codes and 10 in codes                                     # 256000 and 11025 have no code; 48000 has
    # a seek table with a skipped duplicate: 3000 names frame 0 twice
    n = K.CASES["contents_one_clip"][1].shape[1]
    assert K.CASES["contents_one_clip"][3] == 3000 and flacref.seek_frames(n, 3000)[:3] == [0, 1, 2]
    assert len(flacref.seek_frames(n, 3000)) < len(range(0, n, 3000))
    assert flacref.seek_frames(10000, 5000) == [0, 1] and flacref.seek_frames(4097, 4096) == [0, 1] and flacref.seek_frames(4096, 4096) == [0]
    assert flacref.seek_frames(8192 + 33, 48000) == [0] and flacref.seek_frames(5, 1) == [0]


def test_fixed_never_reaches_verbatim_and_verbatim_is_the_bound(built_lib):
    for name in K.CASES:
        for clip in K.reference(name)[2]:
            for f in clip:
                assert f["bits"] <= 8 + 16 * f["bs"] and (f["kind"] != "FIXED" or f["bits"] < 8 + 16 * f["bs"])
    noise = np.random.default_rng(5).integers(-32768, 32768, 3 * 4096 + 77).astype(np.int16)
    for seek in (0, 1000, 4096, 48000):
        assert len(flacref.encode(noise, 48000, seek)) == host.flac_max_bytes(1, noise.size, seek)       # every frame VERBATIM: the bound is met


# ---------------------------------------------------------------------------------------------------- the decoder's rejections
@pytest.fixture(scope="module")
def stream():
    x = np.concatenate([K.content("walk40"), K.content("noise3"), K.content("sine100")[:500]])
    s = flacref.encode(x, 48000, 3000)
    y, info = flacdec.decode(s)
    assert np.array_equal(y, x) and len(info["seek"]) == 2                 # 0 and 3000 share frame 0
    return s, info


def refresh(frame):
    """A frame with its header or body changed, both CRCs made right again (header: 4 + 1 number byte [+ 2 block size])."""
    hb = 5 + (2 if frame[2] >> 4 == 7 else 1 if frame[2] >> 4 == 6 else 0)
    head = frame[:hb] + bytes([flacdec.crc8(frame[:hb])])
    body = head + frame[hb + 1:-2]
    return body + flacdec.crc16(body).to_bytes(2, "big")


def with_frame(s, info, i, edit):
    m = info["frames"][i]
    a, b = m["start"], m["start"] + m["bytes"]
    fr = bytearray(s[a:b])
    edit(fr)
    return s[:a] + refresh(bytes(fr)) + s[b:]


def flip(s, pos, mask):
    b = bytearray(s)
    b[pos] ^= mask
    return bytes(b)


def test_decoder_rejects_each_corruption(stream):
    s, info = stream
    f0, f1, f2 = (m["start"] for m in info["frames"])
    audio = f0

    def bad(t, what):
        with pytest.raises(flacdec.FlacError, match=what):
            flacdec.decode(t)

    bad(flip(s, f1, 0x01), "sync")
    bad(flip(s, f1 + 1, 0x04), "sync")
    bad(flip(s, f1 + 5, 0x01), "CRC-8")
    bad(flip(s, f1 + 2, 0x01), "CRC-8|STREAMINFO")                       # another rate code
    bad(flip(s, f1 + 40, 0x20), "CRC-16")
    bad(flip(s, f2 - 1, 0x01), "CRC-16")

    def set_number(fr):
        fr[4] = 5
    bad(with_frame(s, info, 1, set_number), "consecutive")

    def set_reserved_sync(fr):
        fr[1] |= 0x02
    bad(with_frame(s, info, 1, set_reserved_sync), "reserved")

    def set_reserved_head(fr):
        fr[3] |= 0x01
    bad(with_frame(s, info, 1, set_reserved_head), "reserved")

    bad(s[:4 + 4 + 13] + flip(s[4 + 4 + 13:], 4, 0x01), "STREAMINFO says")                 # total samples + 1
    bad(flip(s, 4 + 4 + 6, 0x01), "frame sizes")                                             # min frame size
    bad(flip(s, 4 + 4 + 9, 0x01), "frame sizes|past the end")                                # max frame size
    seek0 = 4 + 4 + 34 + 4
    bad(flip(s, seek0 + 18 + 15, 0x01), "seek point")                                        # the second point's offset
    bad(flip(s, seek0 + 18 + 7, 0x01), "seek point")                                         # its sample number
    bad(flip(s, seek0 + 18 + 17, 0x01), "seek point")                                        # its sample count
    bad(s[:-1], "truncated|past the end")
    bad(b"fLaX" + s[4:], "marker")
    assert audio == seek0 + 2 * 18


def test_decoder_rejects_non_zero_padding():
    """A frame whose subframe ends off a byte boundary, a padding bit set and both CRCs made right."""
    x = K.content("noise3")
    s, info = flacref.encode(x, 48000, info=True)
    assert info[0]["bits"] % 8 != 0
    _, dinfo = flacdec.decode(s)

    def set_padding(fr):
        fr[-3] |= 0x01
    t = with_frame(s, dinfo, 0, set_padding)
    assert t != s
    with pytest.raises(flacdec.FlacError, match="padding"):
        flacdec.decode(t)


def test_decoder_reads_what_the_encoder_never_writes():
    """Rice method 1, an escape partition, wasted bits and the block-size and rate codes our encoder does not use, hand-assembled."""
    def frame(head_tail, fields, bs_code, rate_code, extra=b""):
        h = bytes([0xFF, 0xF8, (bs_code << 4) | rate_code, 0x08, 0]) + extra
        h += bytes([flacdec.crc8(h)])
        bits = "".join(format(v & ((1 << ln) - 1), f"0{ln}b") for ln, v in fields)      # (a packer of its own: nothing of flacref)
        bits += "0" * (-len(bits) % 8)
        body = h + int(bits, 2).to_bytes(len(bits) // 8, "big")
        return body + flacdec.crc16(body).to_bytes(2, "big")

    def stream_of(fr, n, rate, bs):
        si = (bs.to_bytes(2, "big") * 2 + len(fr).to_bytes(3, "big") * 2 + ((rate << 44) | (15 << 36) | n).to_bytes(8, "big") + bytes(16))
        return b"fLaC" + bytes([0x80]) + (34).to_bytes(3, "big") + si + fr

    x = [3, -2, 7, 100, -100, 0, 1, -1] + [5] * 184                      # 192 samples: block-size code 1
    # FIXED order 1, method 1 (5-bit parameters), partition order 0, escape with 9 raw bits
    res = [b - a for a, b in zip(x[:-1], x[1:])]
    fields = [(8, (8 | 1) << 1), (16, x[0]), (2, 1), (4, 0), (5, 31), (5, 9)] + [(9, r) for r in res]
    y, info = flacdec.decode(stream_of(frame(None, fields, 1, 9), 192, 44100, 192))
    assert y.tolist() == x and info["frames"][0]["method"] == 1 and info["frames"][0]["ks"] == [31]
    # VERBATIM with two wasted bits, the 16-bit rate-in-Hz code, the 8-bit block size code
    v = [4 * a for a in (1, -3, 100, -8000, 8191, 0, 2, -2, 9, 17)]
    fields = [(8, 0x03), (2, 0b01)] + [(14, a >> 2) for a in v]
    y, info = flacdec.decode(stream_of(frame(None, fields, 6, 13, bytes([9, 11025 >> 8, 11025 & 255])), 10, 11025, 16))
    assert y.tolist() == v and info["frames"][0]["wasted"] == 2


# ---------------------------------------------------------------------------------------------------- C ABI, no device needed
def test_flac_symbols_are_exported(built_lib):
    lib = host.load_library()
    for s in ENTRIES:
        assert s in host.SYMBOLS and getattr(lib, s)
    assert birdnet_go_amd.encode_clips is flac.encode_clips and birdnet_go_amd.normalize_and_encode is flac.normalize_and_encode


def test_go_shim_declares_and_binds_the_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shim_dir = os.path.join(root, "birdnet-go_amd", "go", "internal", "inference", "hip")
    shim = open(os.path.join(shim_dir, "backend_hip.go")).read()
    stub = open(os.path.join(shim_dir, "stub_nohip.go")).read()
    assert '"bnhip_flac_max_bytes"' in shim and '"bnhip_flac_encode_pcm16"' in shim and '"bnhip_loudness_flac_pcm16"' in shim
    for fn in ("func EncodeFLAC(pcm []int16, nClips, sampleRate int, gainDB []float64, seekInterval, device int) ([][]byte, error)",
               "func NormalizeAndEncodeFLAC(pcm []int16, nClips, sampleRate int, opts LoudnessOptions, seekInterval, device int) (streams [][]byte, res []Loudness, err error)"):
        b = shim[shim.index(fn):]
        b = b[:b.index("\n}\n")]
        assert "runtime.LockOSThread()" in b and "defer runtime.UnlockOSThread()" in b, fn
        assert re.search(r"lastError\(\)", b), fn
    assert "func EncodeFLAC([]int16, int, int, []float64, int, int) ([][]byte, error)" in stub
    assert "func NormalizeAndEncodeFLAC([]int16, int, int, LoudnessOptions, int, int) ([][]byte, []Loudness, error)" in stub


def test_flac_argument_errors_before_any_device(built_lib):
    lib = host.load_library()
    ci, cd, vp, sz = C.c_int, C.c_double, C.c_void_p, C.c_size_t
    buf = np.zeros(4096, np.int16)
    outb = np.zeros(1 << 16, np.uint8)
    offs = np.zeros(8, np.uint64)
    res = (host.Loudness * 4)()
    fac = np.ones(4, np.float64)
    p, o, f, q, r = vp(buf.ctypes.data), vp(outb.ctypes.data), vp(offs.ctypes.data), vp(fac.ctypes.data), vp(C.addressof(res))
    dev = ci(99)                                                             # no such device: a valid call would fail differently
    cap = host.flac_max_bytes(1, 1024, 0)

    def pcm16(pcm=p, n_clips=1, n=1024, rate=48000, factor=vp(), seek=0, out=o, out_cap=cap, offsets=f):
        return lib.bnhip_flac_encode_pcm16(dev, pcm, ci(n_clips), ci(n), ci(rate), factor, ci(seek), out, sz(out_cap), offsets)

    def device(pcm=p, n_clips=1, n=1024, rate=48000, factor=vp(), seek=0, out=o, out_cap=cap, offsets=f, ws=p, ws_bytes=1 << 20):
        return lib.bnhip_flac_encode_device(dev, pcm, ci(n_clips), ci(n), ci(rate), factor, ci(seek), out, sz(out_cap), offsets, ws, sz(ws_bytes), vp())

    def fused(pcm=p, n_clips=1, n=1024, rate=48000, t=-23.0, c=-1.0, g=30.0, seek=0, res=r, out=o, out_cap=cap, offsets=f):
        return lib.bnhip_loudness_flac_pcm16(dev, pcm, ci(n_clips), ci(n), ci(rate), cd(t), cd(c), cd(g), ci(0), ci(seek), res, out, sz(out_cap), offsets)

    for fn in (pcm16, device, fused):
        assert fn(pcm=vp()) == host.E_INVALID and lib.bnhip_last_error() == b"NULL/empty argument"
        assert fn(out=vp()) == host.E_INVALID and fn(offsets=vp()) == host.E_INVALID
        for bad in (0, -1, 65536):
            assert fn(n_clips=bad) == host.E_INVALID and b"n_clips" in lib.bnhip_last_error()
        assert fn(n=0) == host.E_INVALID and b"n must be" in lib.bnhip_last_error()
        assert fn(seek=-1) == host.E_INVALID and b"seek_interval" in lib.bnhip_last_error()
        assert fn(out_cap=cap - 1) == host.E_INVALID and b"out_cap" in lib.bnhip_last_error()
        assert lib.bnhip_last_error() == b"out_cap smaller than bnhip_flac_max_bytes"                        # (the ragged form names its own)
        assert fn(seek=100, out_cap=cap) == host.E_INVALID and b"out_cap" in lib.bnhip_last_error()       # the seek table counts
        assert fn() != host.BNHIP_OK and b"out_cap" not in lib.bnhip_last_error()                            # valid arguments reach the device check
    for fn in (pcm16, device):
        for bad in (0, -5, 1048576):
            assert fn(rate=bad) == host.E_INVALID and b"sample rate" in lib.bnhip_last_error()
    for bad in (0, 7999):
        assert fused(rate=bad) == host.E_INVALID and b"sample rate too low" in lib.bnhip_last_error()
    assert fused(rate=1048576) == host.E_INVALID and b"sample rate" in lib.bnhip_last_error()
    assert fused(res=vp()) == host.E_INVALID
    for bad in (math.nan, INF, 0.0):
        assert fused(t=bad) == host.E_INVALID and b"target loudness" in lib.bnhip_last_error()
    assert fused(c=1.0) == host.E_INVALID and fused(g=math.nan) == host.E_INVALID
    for bad in (math.nan, INF, -INF, -0.5):
        fac[0] = bad
        assert pcm16(factor=q) == host.E_INVALID and b"factor" in lib.bnhip_last_error()
    fac[0] = 1.0
    assert device(ws=vp()) == host.E_INVALID
    assert device(ws_bytes=16) == host.E_INVALID and b"workspace" in lib.bnhip_last_error()
    odd = buf.ctypes.data + 2 if (buf.ctypes.data + 2) % 256 else buf.ctypes.data + 4
    assert device(ws=vp(odd)) == host.E_INVALID and b"aligned" in lib.bnhip_last_error()
    need = sz(0)
    assert lib.bnhip_flac_workspace_size(ci(3), ci(48000), C.byref(need)) == host.BNHIP_OK and need.value > 0
    assert host.flac_workspace_size(3, 48000) == need.value
    assert lib.bnhip_flac_workspace_size(ci(3), ci(48000), None) == host.E_INVALID
    assert lib.bnhip_flac_workspace_size(ci(0), ci(48000), C.byref(need)) == host.E_INVALID
    assert lib.bnhip_flac_max_bytes(ci(3), ci(48000), ci(0), None) == host.E_INVALID
    assert lib.bnhip_flac_max_bytes(ci(3), ci(0), ci(0), C.byref(need)) == host.E_INVALID
    assert lib.bnhip_flac_max_bytes(ci(3), ci(48000), ci(-1), C.byref(need)) == host.E_INVALID
    assert lib.bnhip_flac_max_bytes(ci(3), ci(4096), ci(0), C.byref(need)) == host.BNHIP_OK
    assert need.value == 3 * (42 + 4 + 1 + 1 + 1 + 2 * 4096 + 2)             # header; sync + codes, number, CRC-8, subframe byte, samples, CRC-16


def test_only_mono_int16_is_supported(built_lib):
    for call in (lambda: host.flac_encode(np.zeros(100, np.int16), 48000, channels=2),
                 lambda: host.loudness_flac(np.zeros(100, np.int16), 48000, channels=2),
                 lambda: host.flac_encode(np.zeros(100, np.float32), 48000),
                 lambda: host.loudness_flac(np.zeros(100, np.int32), 48000),
                 lambda: flac.encode_clips([np.zeros((50, 2), np.int16)], 48000),
                 lambda: flac.normalize_and_encode([np.zeros(50, np.float32)], 48000)):
        with pytest.raises(host.HipError) as e:
            call()
        assert e.value.code == host.E_UNSUPPORTED
