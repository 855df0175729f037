"""The ragged spectrogram entries without a device (bnhip_spectrogram_ragged_*, bnhip_spectrogram_png_ragged_pcm16): the symbols and
their declarations, the workspace size against its documented formula, the argument errors answered before any device is touched,
generate_burst's argument checks and grouping with the render stubbed, and the bursts of tests/specraggedcases.py themselves (they
reach what they are there for, and the restatement of the compared ones stays inside specref.compare's tie cap)."""
import ctypes as C
import os

import numpy as np
import pytest

import specraggedcases as K
import specref
from birdnet_go_amd import host, spectrogram as sg

ENTRIES = ("bnhip_spectrogram_ragged_workspace_size", "bnhip_spectrogram_ragged_pcm16", "bnhip_spectrogram_png_ragged_pcm16",
           "bnhip_spectrogram_ragged_device")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bnhip.h")


def test_symbols_are_exported_and_declared(built_lib):
    lib = C.CDLL(built_lib)
    with open(HEADER) as fh:
        header = fh.read()
    for s in ENTRIES:
        assert s in host.SYMBOLS and hasattr(lib, s), s
        assert f"int {s}(" in header, s
    assert "bnhip_spectrogram_* take equally long clips" not in header


@pytest.mark.parametrize("name", list(K.BURSTS))
def test_workspace_size_is_the_documented_formula(built_lib, name):
    width, height, lens = K.BURSTS[name]
    lib, b = host.load_library(), C.c_size_t(0)              # (the entry itself: the bursts carry heights the wrapper would not derive)
    x = np.array(lens, np.int32)
    lib.bnhip_spectrogram_ragged_workspace_size.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
    assert lib.bnhip_spectrogram_ragged_workspace_size(x.size, x.ctypes.data, width, height, C.byref(b)) == host.BNHIP_OK
    assert b.value == K.workspace_bytes(len(lens)) and b.value % 256 == 0 and b.value >= 24 * len(lens)
    assert K.workspace_bytes(10) == 256 and K.workspace_bytes(11) == 512 and K.workspace_bytes(300) == 7424
    if name == "a":
        assert host.spectrogram_ragged_workspace_size(lens, width) == b.value


def test_errors_before_any_device(built_lib):
    lib = host.load_library()
    ci, cd, vp, sz = C.c_int, C.c_double, C.c_void_p, C.c_size_t
    W, H = 258, 129
    buf, img, offs = np.zeros(4096, np.int16), np.zeros(2 * H * W, np.uint8), np.zeros(8, np.uint64)
    cap0 = host.png_max_bytes(2, W, H)
    outb, pal = np.zeros(cap0, np.uint8), np.zeros(768, np.uint8)
    wsb = np.zeros(4096 + 256, np.uint8)
    aligned = (wsb.ctypes.data + 255) & ~255
    dev = ci(99)                                                             # no such device: a valid call fails differently, later
    good = np.array([1000, 24], np.int32)
    b = sz(0)
    hann = specref.hann(256)

    def run(which, lens=good, n_clips=None, width=W, height=H, window=None, top=0.0, rng=100.0, pcm=vp(buf.ctypes.data), cap=cap0,
            ws=256, wsp=aligned, rate_in=24000, rate_out=0):
        L = vp(lens.ctypes.data) if lens is not None else vp()
        nc = ci(len(lens) if n_clips is None else n_clips)
        wn = vp(window.ctypes.data) if window is not None else vp()
        if which == "ws":
            return lib.bnhip_spectrogram_ragged_workspace_size(nc, L, ci(width), ci(height), C.byref(b))
        if which == "pcm16":
            return lib.bnhip_spectrogram_ragged_pcm16(dev, pcm, nc, L, ci(rate_in), ci(rate_out), ci(width), ci(height), wn, cd(top), cd(rng),
                                                      vp(img.ctypes.data))
        if which == "png":
            return lib.bnhip_spectrogram_png_ragged_pcm16(dev, pcm, nc, L, ci(rate_in), ci(rate_out), ci(width), ci(height), wn, cd(top),
                                                          cd(rng), vp(pal.ctypes.data), vp(outb.ctypes.data), sz(cap), vp(offs.ctypes.data))
        assert which == "device"
        return lib.bnhip_spectrogram_ragged_device(dev, pcm, ci(0), nc, L, ci(width), ci(height), wn, cd(top), cd(rng), vp(img.ctypes.data),
                                                   vp(wsp), sz(ws), vp())

    every, renders = ("ws", "pcm16", "png", "device"), ("pcm16", "png", "device")
    err = lambda: lib.bnhip_last_error()
    huge = np.full(40, 2**31 - 1, np.int32)                                  # 40 (2^31 - 1) > 2^36 - 1
    for w in every:
        assert run(w, lens=None, n_clips=2) == host.E_INVALID and err() == b"NULL/empty argument", w
        assert run(w, lens=np.array([5, 0, 7], np.int32)) == host.E_INVALID and b"at least 1" in err(), w
        assert run(w, lens=np.array([5, -3], np.int32)) == host.E_INVALID and b"at least 1" in err(), w
        assert run(w, n_clips=0) == host.E_INVALID and b"n_clips" in err(), w
        assert run(w, lens=np.ones(65536, np.int32)) == host.E_INVALID and b"n_clips" in err(), w
        assert run(w, lens=huge) == host.E_INVALID and b"2^36" in err(), w
        # what the uniform entries reject of the image
        assert run(w, width=0) == host.E_INVALID and b"width" in err(), w
        assert run(w, width=4097) == host.E_INVALID and b"width" in err(), w
        assert run(w, height=130) == host.E_INVALID and b"height" in err(), w
        assert run(w, height=17) == host.E_UNSUPPORTED and b"FFT size" in err(), w          # N = 32
        assert run(w, height=4097) == host.E_UNSUPPORTED and b"FFT size" in err(), w        # N = 8192
    for w in renders:
        bad = hann.copy()
        bad[7] = np.inf
        assert run(w, window=bad) == host.E_INVALID and b"window" in err(), w
        bad[7] = np.nan
        assert run(w, window=bad) == host.E_INVALID and b"window" in err(), w
        assert run(w, rng=0.0) == host.E_INVALID and b"range_db" in err(), w
        assert run(w, rng=-80.0) == host.E_INVALID and b"range_db" in err(), w
        assert run(w, rng=np.nan) == host.E_INVALID and b"range_db" in err(), w
        assert run(w, top=np.inf) == host.E_INVALID and b"top_db" in err(), w
        assert run(w, pcm=vp()) == host.E_INVALID and err() == b"NULL/empty argument", w
    for w in ("pcm16", "png"):
        assert run(w, rate_in=0, rate_out=24000) == host.E_INVALID and b"sample rates" in err(), w
        assert run(w, rate_in=48000, rate_out=-1) == host.E_INVALID and b"sample rates" in err(), w
    assert run("png", cap=cap0 - 1) == host.E_INVALID and b"out_cap" in err()
    # the device entry's workspace: one byte short, misaligned, missing
    assert run("ws") == host.BNHIP_OK and b.value == 256
    assert run("device", ws=255) == host.E_INVALID and b"workspace" in err()
    assert run("device", wsp=aligned + 128, ws=4096) == host.E_INVALID and b"aligned" in err()
    assert run("device", wsp=0) == host.E_INVALID and err() == b"NULL/empty argument"
    # valid arguments go on to the device, which is not there
    for w in renders:
        rc = run(w, window=hann)
        assert rc != host.BNHIP_OK and (rc != host.E_INVALID or b"device ordinal" in err()), w
    for w in ("pcm16", "png"):
        rc = run(w, rate_in=48000, rate_out=24000)
        assert rc != host.BNHIP_OK and (rc != host.E_INVALID or b"device ordinal" in err()), w


# ---- generate_burst with the render stubbed: argument checks, grouping order, input order of the result
class _Stub:
    """Stands in for host.spectrogram / spectrogram_ragged (and their PNG forms): the 'image' of a clip is its first sample, and
    every call is recorded."""

    def __init__(self, monkeypatch):
        self.calls = []
        monkeypatch.setattr(host, "spectrogram_size", lambda width: (3, 4))
        monkeypatch.setattr(host, "spectrogram", self._uniform)
        monkeypatch.setattr(host, "spectrogram_ragged", self._ragged)
        monkeypatch.setattr(host, "spectrogram_png", self._uniform_png)
        monkeypatch.setattr(host, "spectrogram_png_ragged", self._ragged_png)

    @staticmethod
    def _img(clips, width):
        return np.stack([np.full((3, width), int(c[0]) & 0xFF, np.uint8) for c in clips])

    def _uniform(self, clips, rate, width, **kw):
        self.calls.append(("uniform", [int(c[0]) for c in clips], clips.shape[1], kw["rate_out"]))
        return self._img(clips, width)

    def _ragged(self, clips, rate, width, **kw):
        self.calls.append(("ragged", [int(c[0]) for c in clips], None, kw["rate_out"]))
        return self._img(clips, width)

    def _png(self, clips, width, tmp):
        streams = []
        for im in self._img(clips, width):
            path = os.path.join(tmp, "s.png")
            sg.write_png(path, im, sg.palette("default"))
            with open(path, "rb") as fh:
                streams.append(fh.read())
        return streams

    def _uniform_png(self, clips, rate, width, palette, **kw):
        self.calls.append(("uniform_png", [int(c[0]) for c in clips], clips.shape[1], kw["rate_out"]))
        return self._png(clips, width, self.tmp)

    def _ragged_png(self, clips, rate, width, palette, **kw):
        self.calls.append(("ragged_png", [int(c[0]) for c in clips], None, kw["rate_out"]))
        return self._png(clips, width, self.tmp)


def _mini_burst():
    lens = (7, 3, 7, 5, 3, 7)
    return [np.full(n, 10 + i, np.int16) for i, n in enumerate(lens)]


def test_generate_burst_groups_by_length_in_input_order(monkeypatch, tmp_path):
    stub = _Stub(monkeypatch)
    stub.tmp = str(tmp_path)
    clips = _mini_burst()
    paths = [str(tmp_path / f"c{i}.png") for i in range(len(clips))]
    got = sg.generate_burst(clips, paths, 8, 48000)
    # one call per length, lengths in the order they first appear, clips of a length in input order
    assert stub.calls == [("uniform", [10, 12, 15], 7, 24000), ("uniform", [11, 14], 3, 24000), ("uniform", [13], 5, 24000)]
    assert got.shape == (6, 3, 8) and got.dtype == np.uint8 and got[:, 0, 0].tolist() == [10, 11, 12, 13, 14, 15]
    for i, p in enumerate(paths):
        with open(p, "rb") as fh:
            assert sg.read_png_indices(fh.read())[0, 0] == 10 + i
    stub.calls.clear()
    got = sg.generate_burst(clips, paths, 8, 48000, ragged=True, profile=sg.FrequencyProfile(0))
    assert stub.calls == [("ragged", [10, 11, 12, 13, 14, 15], None, 0)] and got[:, 0, 0].tolist() == [10, 11, 12, 13, 14, 15]
    stub.calls.clear()
    got = sg.generate_burst(clips, paths, 8, 48000, device_png=True)
    assert [c[0] for c in stub.calls] == ["uniform_png"] * 3 and got[:, 0, 0].tolist() == [10, 11, 12, 13, 14, 15]
    stub.calls.clear()
    got = sg.generate_burst(clips, paths, 8, 48000, device_png=True, ragged=True)
    assert [c[0] for c in stub.calls] == ["ragged_png"] and got[:, 0, 0].tolist() == [10, 11, 12, 13, 14, 15]
    for i, p in enumerate(paths):
        with open(p, "rb") as fh:
            assert sg.read_png_indices(fh.read())[0, 0] == 10 + i


@pytest.mark.parametrize("ragged", [False, True])
def test_generate_burst_argument_checks(monkeypatch, tmp_path, ragged):
    stub = _Stub(monkeypatch)
    clips = _mini_burst()
    paths = [str(tmp_path / f"c{i}.png") for i in range(len(clips))]
    go = lambda c=clips, p=paths, **kw: sg.generate_burst(c, p, 8, kw.pop("rate", 48000), ragged=ragged, **kw)
    for bad in ([], clips[:-1], clips[:2] + [np.zeros(0, np.int16)] + clips[3:], clips[:2] + [np.zeros(4, np.float32)] + clips[3:],
                clips[:2] + [np.zeros((2, 4), np.int16)] + clips[3:]):
        with pytest.raises(ValueError):
            go(c=bad)
    with pytest.raises(ValueError):
        go(p=paths[:-1] + ["relative.png"])
    with pytest.raises(ValueError):
        go(p=paths[:-1] + [""])
    with pytest.raises(ValueError):
        go(dynamic_range="90")
    with pytest.raises(ValueError):
        go(style="sepia")
    with pytest.raises(ValueError):
        go(rate=0)
    assert stub.calls == []                                                  # nothing reached the render


# ---- the bursts themselves
def test_the_bursts_reach_what_they_are_there_for():
    Ks = {name: [K.frames_per_column(n, w, h) for n in lens] for name, (w, h, lens) in K.BURSTS.items()}
    assert sorted(set(Ks["a"])) == [1, 2, 3, 4] and Ks["a"][0] == 2 and Ks["a"][6] == 1          # W N + 1 and W N
    assert K.BURSTS["a"][2][6] == 258 * 256 and K.BURSTS["a"][2][0] == 258 * 256 + 1 and 1 in K.BURSTS["a"][2]
    assert min(K.BURSTS["a"][2][1], K.BURSTS["a"][2][4]) < 256
    starts = np.concatenate([[0], np.cumsum(K.BURSTS["a"][2])])
    assert all(int(s) % 2 for s in starts[1:3]) and any(int(s) % 2 for s in starts[3:-1])
    assert Ks["kbig"] == [65, 2, 71, 1, 1, 64] and max(Ks["kbig"]) > K.SPEC_FMAX and Ks["kbig"][0] != max(Ks["kbig"])
    assert Ks["n4096"] == [2, 1, 1, 1] and Ks["odd"] == [2, 1, 3, 1, 1, 2, 1] and K.BURSTS["odd"][0] % 32 == 1
    assert Ks["n1024"] == [2, 1, 1, 1]
    assert len(K.BURSTS["many"][2]) == 300 and len(set(K.BURSTS["many"][2])) == 257
    assert len(set(K.RESAMPLED["lens"])) == 5
    w, h, clips = K.burst("a")
    assert [c.size for c in clips] == list(K.BURSTS["a"][2]) and all(c.dtype == np.int16 and not c.flags.writeable for c in clips)


@pytest.mark.parametrize("name", K.COMPARED)
def test_restatement_stays_inside_the_tie_cap(name):
    """specref.compare asserts its cap of 1e-4 on the restatement before it looks at the device image: here the restatement is
    compared with itself, so only that assertion can fail.  (`many` is not held to compare: its worst clip has 1.5e-3.)"""
    width, height, clips = K.burst(name)
    worst = 0.0
    for c in clips:
        x = np.asarray(c, np.float64) / 32768.0
        worst = max(worst, specref.compare(specref.render(x, width, height), x, width, height))
    print(f"{name}: worst excused share {worst:.3g}")             # (at most one pixel of a 16 x 2049 image, 3.05e-5, on these bursts)
