"""The ragged entries without a device (bnhip_*_ragged_*): the symbols, the size entries against the uniform ones, the argument
errors answered before any device is touched, the Python packers, and the bursts of tests/raggedcases.py themselves (they reach
what they are there for, and no block energy of theirs sits on a gate)."""
import ctypes as C

import numpy as np
import pytest

import raggedcases as K
from birdnet_go_amd import host

ENTRIES = ("bnhip_loudness_ragged_workspace_size", "bnhip_loudness_ragged_normalize_pcm16", "bnhip_loudness_ragged_normalize_device",
           "bnhip_flac_ragged_max_bytes", "bnhip_flac_ragged_workspace_size", "bnhip_flac_ragged_encode_device",
           "bnhip_flac_ragged_encode_pcm16", "bnhip_loudness_flac_ragged_pcm16")


def test_ragged_symbols_are_exported(built_lib):
    lib = C.CDLL(built_lib)
    for s in ENTRIES:
        assert s in host.SYMBOLS and hasattr(lib, s), s


@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("seek", [0, 8000, 100])
def test_max_bytes_is_the_sum_of_the_clips(built_lib, name, seek):
    lens = K.BUILDERS[name][0]
    assert host.flac_ragged_max_bytes(lens, seek) == sum(host.flac_max_bytes(1, n, seek) for n in lens)


def test_workspace_sizes(built_lib):
    n = K.LENS_C[0]
    for lpc in (0, 8):
        assert host.flac_ragged_workspace_size(K.LENS_C, lpc) >= host.flac_lpc_workspace_size(5, n, lpc) > 0
    assert host.flac_ragged_workspace_size(K.LENS_C, 8) > host.flac_ragged_workspace_size(K.LENS_C, 0)
    assert host.loudness_ragged_workspace_size(K.LENS_C, K.RATE) >= host.loudness_workspace_size(5, n, K.RATE) > 0
    for lens in (K.LENS_A, K.LENS_B, (1,)):
        assert host.flac_ragged_workspace_size(lens, 0) > 0 and host.loudness_ragged_workspace_size(lens, K.RATE) > 0
    # more samples never need less
    assert host.loudness_ragged_workspace_size(K.LENS_A, K.RATE) > host.loudness_ragged_workspace_size(K.LENS_A[:5], K.RATE)
    assert host.flac_ragged_workspace_size(K.LENS_A, 8) > host.flac_ragged_workspace_size(K.LENS_A[:5], 8)


def test_errors_before_any_device(built_lib):
    lib = host.load_library()
    ci, cd, vp, sz = C.c_int, C.c_double, C.c_void_p, C.c_size_t
    buf, outb, offs = np.zeros(4096, np.int16), np.zeros(1 << 16, np.uint8), np.zeros(8, np.uint64)
    res = (host.Loudness * 4)()
    p, o, f, r = vp(buf.ctypes.data), vp(outb.ctypes.data), vp(offs.ctypes.data), vp(C.addressof(res))
    wsb = np.zeros((1 << 20) + 256, np.uint8)
    wsp = vp((wsb.ctypes.data + 255) & ~255)                                 # (the device entries ask for a 256-byte aligned workspace)
    dev = ci(99)                                                             # no such device: a valid call fails differently, later
    good = np.array([1000, 24], np.int32)
    cap = sz(host.flac_ragged_max_bytes(good, 0))
    b = C.c_size_t(0)

    def run(which, lens=good, n_clips=None, rate=8000, seek=0, lpc=0, pcm=p, cap=cap, ws=sz(1 << 20), target=-23.0):
        L = vp(lens.ctypes.data) if lens is not None else vp()
        nc = ci(len(lens) if n_clips is None else n_clips)
        if which == "loud_ws":
            return lib.bnhip_loudness_ragged_workspace_size(nc, L, ci(rate), C.byref(b))
        if which == "loud_pcm16":
            return lib.bnhip_loudness_ragged_normalize_pcm16(dev, pcm, nc, L, ci(rate), cd(target), cd(-1.0), cd(30.0), ci(0), vp(), r)
        if which == "loud_device":
            return lib.bnhip_loudness_ragged_normalize_device(dev, pcm, nc, L, ci(rate), cd(target), cd(-1.0), cd(30.0), ci(0), vp(), r, wsp, ws, vp())
        if which == "flac_max":
            return lib.bnhip_flac_ragged_max_bytes(nc, L, ci(seek), C.byref(b))
        if which == "flac_ws":
            return lib.bnhip_flac_ragged_workspace_size(nc, L, ci(lpc), C.byref(b))
        if which == "flac_device":
            return lib.bnhip_flac_ragged_encode_device(dev, pcm, nc, L, ci(rate), vp(), ci(seek), o, cap, f, wsp, ws, vp(), ci(lpc))
        if which == "flac_pcm16":
            return lib.bnhip_flac_ragged_encode_pcm16(dev, pcm, nc, L, ci(rate), vp(), ci(seek), o, cap, f, ci(lpc))
        assert which == "fused"
        return lib.bnhip_loudness_flac_ragged_pcm16(dev, pcm, nc, L, ci(rate), cd(target), cd(-1.0), cd(30.0), ci(0), ci(seek), r, o, cap, f, ci(lpc))

    every = ("loud_ws", "loud_pcm16", "loud_device", "flac_max", "flac_ws", "flac_device", "flac_pcm16", "fused")
    huge = np.full(40, 2**31 - 1, np.int32)                                  # 40 (2^31 - 1) > 2^36 - 1
    for w in every:
        assert run(w, lens=None, n_clips=2) == host.E_INVALID and lib.bnhip_last_error() == b"NULL/empty argument", w
        assert run(w, lens=np.array([5, 0, 7], np.int32)) == host.E_INVALID and b"at least 1" in lib.bnhip_last_error(), w
        assert run(w, lens=np.array([5, -3], np.int32)) == host.E_INVALID and b"at least 1" in lib.bnhip_last_error(), w
        assert run(w, n_clips=0) == host.E_INVALID and b"n_clips" in lib.bnhip_last_error(), w
        assert run(w, n_clips=65536) == host.E_INVALID and b"n_clips" in lib.bnhip_last_error(), w
        assert run(w, lens=huge) == host.E_INVALID and b"2^36" in lib.bnhip_last_error(), w
    # what the uniform entries reject
    for w in ("loud_ws", "loud_pcm16", "loud_device", "fused"):
        assert run(w, rate=7999) == host.E_INVALID and b"sample rate" in lib.bnhip_last_error(), w
    for w in ("loud_pcm16", "loud_device", "fused"):
        assert run(w, target=0.0) == host.E_INVALID and b"target" in lib.bnhip_last_error(), w
    for w in ("flac_device", "flac_pcm16", "fused"):
        assert run(w, rate=1 << 20) == host.E_INVALID and b"sample rate" in lib.bnhip_last_error(), w
        assert run(w, seek=-1) == host.E_INVALID and b"seek_interval" in lib.bnhip_last_error(), w
        assert run(w, lpc=9) == host.E_INVALID and b"lpc_order" in lib.bnhip_last_error(), w
        assert run(w, cap=sz(cap.value - 1)) == host.E_INVALID and b"out_cap" in lib.bnhip_last_error(), w
        assert lib.bnhip_last_error() == b"out_cap smaller than bnhip_flac_ragged_max_bytes", w      # (each form names its own size entry)
        assert run(w, pcm=vp()) == host.E_INVALID and lib.bnhip_last_error() == b"NULL/empty argument", w
    assert run("flac_ws", lpc=-1) == host.E_INVALID and run("flac_max", seek=-1) == host.E_INVALID
    need = host.flac_ragged_workspace_size(good, 8)
    assert run("flac_device", lpc=8, ws=sz(need - 1)) == host.E_INVALID and b"workspace" in lib.bnhip_last_error()
    assert lib.bnhip_last_error() == b"workspace smaller than bnhip_flac_ragged_workspace_size"
    need = host.loudness_ragged_workspace_size(good, 8000)
    assert run("loud_device", ws=sz(need - 1)) == host.E_INVALID and b"workspace" in lib.bnhip_last_error()
    assert lib.bnhip_last_error() == b"workspace smaller than bnhip_loudness_ragged_workspace_size"
    bad = np.array([1.0, np.nan])
    assert lib.bnhip_flac_ragged_encode_pcm16(dev, p, ci(2), vp(good.ctypes.data), ci(8000), vp(bad.ctypes.data), ci(0), o, cap, f,
                                              ci(0)) == host.E_INVALID and b"factor" in lib.bnhip_last_error()
    # valid arguments go on to the device, which is not there
    for w in ("loud_pcm16", "loud_device", "flac_device", "flac_pcm16", "fused"):
        rc = run(w)
        assert rc != host.BNHIP_OK and (rc != host.E_INVALID or b"device ordinal" in lib.bnhip_last_error()), w
    for w in ("loud_ws", "flac_max", "flac_ws"):
        assert run(w) == host.BNHIP_OK and b.value > 0, w


def test_packers_round_trip_order_and_lengths():
    clips = K.burst("a")
    packed, lens = host.ragged_pack(clips)
    assert packed.dtype == np.int16 and packed.ndim == 1 and packed.size == sum(K.LENS_A)
    assert lens.dtype == np.int32 and lens.tolist() == list(K.LENS_A)
    back = host.ragged_unpack(packed, lens)
    assert len(back) == len(clips) and all(np.array_equal(x, y) for x, y in zip(back, clips))
    start = np.concatenate([[0], np.cumsum(lens)])
    assert all(packed[start[c]] == clips[c][0] and packed[start[c + 1] - 1] == clips[c][-1] for c in range(len(clips)))
    assert any(int(s) % 2 for s in start[1:-1])                              # later clips do start on odd offsets
    for bad, code in (([], host.E_INVALID), ([np.zeros(0, np.int16)], host.E_INVALID), ([np.zeros(4, np.float32)], host.E_UNSUPPORTED),
                      ([np.zeros((2, 4), np.int16)], host.E_UNSUPPORTED)):
        with pytest.raises(host.HipError) as e:
            host.ragged_pack(bad)
        assert e.value.code == code


def test_the_bursts_reach_what_they_are_there_for():
    tiles = lambda n: (n + 16 + 1023) // 1024
    assert sorted({tiles(n) for n in K.LENS_A}) == [1, 5, 9, 13]
    assert sorted({(n + 4095) // 4096 for n in K.LENS_A}) == [1, 2, 3, 4]
    assert {n // K.S for n in K.LENS_A} >= {0, 1, 5, 10, 15} and K.LENS_A[0] < K.S and K.LENS_A[8] < K.S
    assert any(n % 4096 == 0 for n in K.LENS_A) and any(n % 4096 for n in K.LENS_A)
    assert len(K.LENS_B) == 300 and len(set(K.LENS_B)) == 257 and sum(n >= K.S for n in K.LENS_B) == 0
    a = K.burst("a")
    assert not a[5].any() and len(set(a[3].tolist())) == 1 and a[3][0] != 0
    # no block energy of a loudness burst sits on a gate, for the clip as given and for its lifted form
    for name in ("a", "c", "d"):
        for i, (s, m) in enumerate(zip(K.burst(name), K.measurements(name))):
            w = K.loudref.normalize(s, K.RATE, -23.0, -1.0, 60.0, True, m=m)
            assert w["margin"] >= 1e-6, (name, i, w["margin"])
    d = [K.loudref.normalize(s, K.RATE, -23.0, -1.0, 60.0, True, m=m) for s, m in zip(K.burst("d"), K.measurements("d"))]
    lifted = [bool(w["flags"] & K.loudref.GATE_LIFTED) for w in d]
    assert any(lifted) and not all(lifted) and any(w["gain_db"] != 0.0 for w in d)
