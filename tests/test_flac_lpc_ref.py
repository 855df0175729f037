"""The LPC predictors of the FLAC encoder on the CPU: the restatement of the spec (tests/flaclpcref.py) against an independent decoder
written from RFC 9639 (tests/flaclpcdec.py), the branches the shared cases (tests/flaclpccases.py) reach - asserted, so that a later
change of the cases cannot lose one silently - the decoder's own rejections, and the new C ABI entries' argument errors (answered
before any device is touched).

One branch of the spec no int16 frame reaches: the recursion's stop on `err <= 0`.  R is the autocorrelation of a finite integer
sequence, so the exact err of order m is at least the square of the first non-zero windowed sample, and the samples' 16 bits leave
err / R[0] above 1e-11 on any predictable signal; fp64 would have to lose 1 - k^2, i.e. err_m / err_(m-1) < 2^-53.  A search over
5000 structured and random frames (sines, ramps, alternations, decays, sparse noise; 2 to 4096 samples) found no stop.  The guard
stays in the spec and the kernel; test_recursion_stops_when_the_error_is_used_up drives it with a singular R instead."""
import ctypes as C
import os

import numpy as np
import pytest

import birdnet_go_amd  # noqa: F401
from birdnet_go_amd import flac, host

import flaccases
import flacdec
import flaclpccases as K
import flaclpcdec
import flaclpcref
import flacref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENTRIES = ("bnhip_flac_lpc_workspace_size", "bnhip_flac_lpc_encode_device", "bnhip_flac_lpc_encode_pcm16", "bnhip_loudness_flac_lpc_pcm16")


@pytest.mark.parametrize("name", list(K.CASES))
def test_decoder_returns_the_gained_input(built_lib, name):
    rate, clips, _, seek, _ = K.CASES[name]
    buf, off, infos, gained = K.reference(name)
    assert int(off[-1]) <= host.flac_max_bytes(len(clips), clips.shape[1], seek)
    for c, g in enumerate(gained):
        s = buf[int(off[c]):int(off[c + 1])]
        y, info = flaclpcdec.decode(s)
        assert np.array_equal(y, g.astype(np.int64)) and info["rate"] == rate, (name, c)
        for want, got in zip(infos[c], info["frames"]):
            assert (want["kind"], want["bs"], want["bytes"]) == (got["kind"], got["bs"], got["bytes"]), (name, c)
            if want["kind"] == "LPC":
                assert (want["order"], want["porder"], want["ks"]) == (got["order"], got["porder"], got["ks"]) and got["precision"] == 12
                assert all(-2048 <= q <= 2047 for q in got["coefs"]) and 0 <= got["shift"] <= 15


@pytest.mark.parametrize("name", list(K.CONTENTS))
def test_each_content_reaches_its_branch(name):
    want = K.CONTENTS[name][1]
    _, info = flaclpcref.encode(K.content(name), 48000, 0, 8, info=True)
    f = info[0]
    assert f["kind"] == want[0], (name, f)
    if want[0] == "LPC" and want[1] is not None:
        assert f["order"] == want[1], (name, f)


def test_the_cases_reach_every_branch():
    frames = [(K.CASES[name][4], f) for name in K.CASES for clip in K.reference(name)[2] for f in clip]
    kinds = {f["kind"] for _, f in frames}
    assert kinds == {"CONSTANT", "FIXED", "LPC", "VERBATIM"}
    assert {f["order"] for _, f in frames if f["kind"] == "LPC"} == set(range(1, 9))                  # every order wins somewhere
    assert {M for M, _ in frames} == {1, 4, 8}
    for M in (1, 4):                                                                                    # the cap is the winner somewhere
        assert any(f["kind"] == "LPC" and f["order"] == M for m, f in frames if m == M)
    assert any(f["kind"] == "LPC" and f["porder"] > 0 for _, f in frames)
    seen = [(f, f["lpc"]) for _, f in frames if f["lpc"] is not None]
    assert any(f["kind"] == "FIXED" and s["offered"] for f, s in seen)                                 # FIXED beats offered LPC orders
    assert any(f["kind"] == "VERBATIM" and s["offered"] for f, s in seen)
    assert any(s["R0"] == 0 and not s["offered"] for _, s in seen)                                      # not constant, yet R[0] == 0
    assert any(s["R0"] > 0 and s["reached"] > 0 and len(s["not_offered"]) == s["reached"] for _, s in seen)   # every coefficient zero
    assert any(15 in s["shifts"].values() for _, s in seen)                                             # the shift's clamp
    assert any(0 < min(s["shifts"].values(), default=99) < 15 for _, s in seen)
    assert any(f["lpc"]["mmax"] < M for M, f in frames if f["lpc"] is not None)                          # bs - 1 < M
    assert {f["bs"] for _, f in frames} >= {1, 2, 3, 5, 9, 16, 17, 33, 64, 255, 256, 257, 4095, 4096}
    assert not any(s["stopped"] or s["over"] for _, s in seen)                                         # (the module's docstring)


def test_recursion_stops_when_the_error_is_used_up():
    """R[1] == R[0]: k = 1, err = 0.  Order 1 is still offered (a_1 = 1 -> 1024 >> 10), the higher orders are not."""
    orders, stopped = flaclpcref.levinson([4, 4, 4, 4, 4], 4)
    assert stopped and orders == {1: [1.0]} and flaclpcref.quantise(orders[1]) == ([1024], 10)
    orders, stopped = flaclpcref.levinson([4, 2, 1, 0, 0], 4)
    assert not stopped and sorted(orders) == [1, 2, 3, 4]
    assert flaclpcref.levinson([0, 0, 0], 2) == ({}, False)
    assert flaclpcref.quantise([0.0, 0.0]) is None and flaclpcref.quantise([float("inf")]) is None and flaclpcref.quantise([float("nan"), 1.0]) is None
    assert flaclpcref.quantise([4096.0]) is None                                                        # a negative shift
    assert flaclpcref.quantise([0.5, -0.5]) == ([1024, -1024], 11)
    assert flaclpcref.quantise([1e-9]) == ([0], 15)
    assert flaclpcref.quantise([0.999999]) == ([2047], 11)                                              # the coefficient's clamp
    assert flaclpcref.quantise([0.3, 0.3, 0.3])[0] == [1229, 1229, 1228]                                 # the error is fed forward


def test_window_and_autocorrelation_bounds():
    for bs in (1, 2, 255, 4095, 4096):
        w = flaclpcref.window(bs)
        assert w.min() >= 1 and w.max() <= 1 << 14 and np.array_equal(w, w[::-1])
    x = np.where(np.arange(4096) % 2 == 0, -32768, 32767).astype(np.int64)
    R = flaclpcref.autocorrelation(x, 8)
    assert 0 < R[0] < 1 << 58 and all(abs(r) <= R[0] for r in R)


@pytest.mark.parametrize("name", ["contents_one_clip", "len17", "len257", "rate11025", "sixty_five"])
def test_order_zero_is_the_encoder_without_lpc(name):
    rate, clips, factor, seek = flaccases.CASES[name]
    want, want_off, _, gained = flaccases.reference(name)
    for c in range(min(len(clips), 5)):
        assert flaclpcref.encode(gained[c], rate, seek, 0) == want[int(want_off[c]):int(want_off[c + 1])]
    got, off = flaclpcref.encode_batch(clips[:5], rate, None if factor is None else factor[:5], seek, 0)
    assert got == want[:int(want_off[min(len(clips), 5)])] and off.tolist() == want_off[:len(off)].tolist()


def test_tawny_owl_is_smaller_with_lpc():
    """The reference's own recording, 40 frames at 16 bits."""
    pcm = K.owl_pcm16(GOLDEN)
    without = flacref.encode(pcm, 48000)
    with_lpc, info = flaclpcref.encode(pcm, 48000, 0, 8, info=True)
    assert np.array_equal(flaclpcdec.decode(with_lpc)[0], pcm.astype(np.int64))
    wins = sum(f["kind"] == "LPC" for f in info)
    print(f"tawny owl, 40 frames at 16 bits: {len(without) / (2.0 * pcm.size):.4f} of the PCM without LPC, "
          f"{len(with_lpc) / (2.0 * pcm.size):.4f} with orders 1..8; LPC wins {wins} of {len(info)} frames")
    assert len(with_lpc) < len(without)
    assert flaclpcref.encode(pcm[:3 * 4096], 48000, 0, 0) == flacref.encode(pcm[:3 * 4096], 48000)


# ---------------------------------------------------------------------------------------------------- the decoder's own rejections
def _lpc_stream(precision_code=11, shift=10, coefs=(1024,), order=1, warm=(5,), bs=16):
    """A one-frame stream: an LPC subframe whose residuals are all zero (k = 0: sixteen `1` bits less the warm-up)."""
    bits = "0" + format(32 | (order - 1), "06b") + "0"
    bits += "".join(format(v & 0xFFFF, "016b") for v in warm)
    bits += format(precision_code, "04b") + format(shift & 31, "05b")
    bits += "".join(format(c & ((1 << (precision_code + 1)) - 1), f"0{precision_code + 1}b") for c in coefs)
    bits += "00" + "0000" + "0000" + "1" * (bs - order)
    bits += "0" * (-len(bits) % 8)
    head = bytes([0xFF, 0xF8, (6 << 4) | 10, 0x08, 0, bs - 1])
    head += bytes([flacdec.crc8(head)])
    fr = head + int(bits, 2).to_bytes(len(bits) // 8, "big")
    fr += flacdec.crc16(fr).to_bytes(2, "big")
    si = (bs.to_bytes(2, "big") * 2 + len(fr).to_bytes(3, "big") * 2 + ((48000 << 44) | (15 << 36) | bs).to_bytes(8, "big") + bytes(16))
    return b"fLaC" + bytes([0x80]) + (34).to_bytes(3, "big") + si + fr


def test_decoder_reads_and_rejects_lpc_subframes():
    y, info = flaclpcdec.decode(_lpc_stream())
    assert y.tolist() == [5] * 16 and info["frames"][0]["kind"] == "LPC" and info["frames"][0]["shift"] == 10
    y, _ = flaclpcdec.decode(_lpc_stream(coefs=(2047, -1024), order=2, warm=(100, 100), shift=10))          # 100 * 1023 >> 10 = 99
    assert y.tolist()[:4] == [100, 100, 99, 99 * 2047 - 100 * 1024 >> 10]
    with pytest.raises(flacdec.FlacError, match="precision"):
        flaclpcdec.decode(_lpc_stream(precision_code=15, coefs=(1024,)))
    with pytest.raises(flacdec.FlacError, match="negative"):
        flaclpcdec.decode(_lpc_stream(shift=-1))
    with pytest.raises(flacdec.FlacError, match="LPC"):                                                  # (the decoder without LPC refuses)
        flacdec.decode(_lpc_stream())
    good = bytearray(_lpc_stream())
    good[-1] ^= 1
    with pytest.raises(flacdec.FlacError, match="CRC-16"):
        flaclpcdec.decode(bytes(good))
    # what flacdec decodes, this one decodes to the same samples
    s = flaccases.reference("len257")
    a, b = flacdec.decode(s[0][:int(s[1][1])]), flaclpcdec.decode(s[0][:int(s[1][1])])
    assert np.array_equal(a[0], b[0]) and [m["kind"] for m in a[1]["frames"]] == [m["kind"] for m in b[1]["frames"]]


# ---------------------------------------------------------------------------------------------------- C ABI, no device needed
def test_lpc_symbols_are_exported(built_lib):
    lib = host.load_library()
    for s in ENTRIES:
        assert s in host.SYMBOLS and getattr(lib, s)
    assert flac.LEVEL5_LPC_ORDER == 8


def test_go_shim_binds_the_lpc_entries():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shim_dir = os.path.join(root, "birdnet-go_amd", "go", "internal", "inference", "hip")
    shim = open(os.path.join(shim_dir, "backend_hip.go")).read()
    stub = open(os.path.join(shim_dir, "stub_nohip.go")).read()
    assert '"bnhip_flac_lpc_encode_pcm16"' in shim and '"bnhip_loudness_flac_lpc_pcm16"' in shim
    fn = "func EncodeFLACLPC(pcm []int16, nClips, sampleRate int, gainDB []float64, seekInterval, lpcOrder, device int) ([][]byte, error)"
    b = shim[shim.index(fn):]
    b = b[:b.index("\n}\n")]
    assert "runtime.LockOSThread()" in b and "defer runtime.UnlockOSThread()" in b and "lastError()" in b
    assert "C.int(opts.LPCOrder)" in shim and "LPCOrder     int" in shim and "LPCOrder     int" in stub
    assert "func EncodeFLACLPC([]int16, int, int, []float64, int, int, int) ([][]byte, error)" in stub
    assert "const Level5LPCOrder = 8" in shim and "const Level5LPCOrder = 8" in stub


def test_lpc_order_errors_before_any_device(built_lib):
    lib = host.load_library()
    ci, cd, vp, sz = C.c_int, C.c_double, C.c_void_p, C.c_size_t
    buf, outb, offs = np.zeros(4096, np.int16), np.zeros(1 << 16, np.uint8), np.zeros(8, np.uint64)
    res = (host.Loudness * 4)()
    p, o, f, r = vp(buf.ctypes.data), vp(outb.ctypes.data), vp(offs.ctypes.data), vp(C.addressof(res))
    dev = ci(99)                                                             # no such device: a valid call would fail differently
    cap = sz(host.flac_max_bytes(1, 1024, 0))

    def pcm16(M, pcm=p):
        return lib.bnhip_flac_lpc_encode_pcm16(dev, pcm, ci(1), ci(1024), ci(48000), vp(), ci(0), o, cap, f, ci(M))

    def device(M, pcm=p):
        return lib.bnhip_flac_lpc_encode_device(dev, pcm, ci(1), ci(1024), ci(48000), vp(), ci(0), o, cap, f, p, sz(1 << 20), vp(), ci(M))

    def fused(M, pcm=p):
        return lib.bnhip_loudness_flac_lpc_pcm16(dev, pcm, ci(1), ci(1024), ci(48000), cd(-23.0), cd(-1.0), cd(30.0), ci(0), ci(0), r, o, cap, f, ci(M))

    for fn in (pcm16, device, fused):
        for bad in (9, -1, 1 << 20):
            assert fn(bad) == host.E_INVALID and b"lpc_order" in lib.bnhip_last_error()
        assert fn(8, pcm=vp()) == host.E_INVALID and lib.bnhip_last_error() == b"NULL/empty argument"
        for M in (0, 8):
            assert fn(M) != host.BNHIP_OK and b"lpc_order" not in lib.bnhip_last_error()               # a valid order goes on to the next check
    need = sz(0)
    for bad in (9, -1):
        assert lib.bnhip_flac_lpc_workspace_size(ci(3), ci(48000), ci(bad), C.byref(need)) == host.E_INVALID
    assert lib.bnhip_flac_lpc_workspace_size(ci(3), ci(48000), ci(8), None) == host.E_INVALID
    assert lib.bnhip_flac_lpc_workspace_size(ci(0), ci(48000), ci(8), C.byref(need)) == host.E_INVALID
    assert host.flac_lpc_workspace_size(3, 48000, 0) == host.flac_workspace_size(3, 48000)
    frames = 3 * 12
    assert host.flac_lpc_workspace_size(3, 48000, 8) == host.flac_lpc_workspace_size(3, 48000, 1) == host.flac_workspace_size(3, 48000) + ((frames * 20 + 255) // 256) * 256
    with pytest.raises(host.HipError) as e:
        host.flac_encode(np.zeros(100, np.int16), 48000, lpc_order=9, device=99)
    assert e.value.code == host.E_INVALID
    with pytest.raises(host.HipError) as e:
        flac.normalize_and_encode([np.zeros(100, np.int16)], 48000, lpc_order=-1, device=99)
    assert e.value.code == host.E_INVALID
