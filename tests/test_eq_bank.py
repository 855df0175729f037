"""The equalizer bank (bnhip_eq_bank_*, bnhip_eq_design, bnhip_windows_write_equalized): the analysis route's EQ chain + gain
(AudioRouter.applyProcessing, internal/audiocore/router.go:1006-1080) for many sources in one device call, byte for byte
against the float64 restatement in tests/eqref.py; the designer against Python's math; the chain builder against
equalizer/builder_test.go's behaviours."""
import ctypes as C

import numpy as np
import pytest

import eqref
from birdnet_go_amd import host
from birdnet_go_amd import stream as S

RATES = (32000, 44100, 48000)
STOCK = {"enabled": True, "filters": [{"type": "HighPass", "frequency": 100, "q": 0.7, "passes": 0},
                                      {"type": "LowPass", "frequency": 15000, "q": 0.7, "passes": 0}]}


def _params(kind, rng):
    f = float(rng.uniform(40, 12000))
    return dict(frequency=f, q=float(rng.uniform(0.3, 4.0)), width=float(rng.uniform(5, 2 * f)), gain=float(rng.uniform(-15, 15)))


# ------------------------------------------------------------------------------------------------ CPU
def test_symbols_exported_and_listed(built_lib):
    lib = C.CDLL(built_lib)
    for f in ("bnhip_eq_bank_create", "bnhip_eq_bank_add_stream", "bnhip_eq_bank_remove_stream", "bnhip_eq_bank_set_chain",
              "bnhip_eq_bank_reset", "bnhip_eq_bank_process_pcm16", "bnhip_windows_write_equalized", "bnhip_eq_design",
              "bnhip_eq_bank_destroy"):
        assert hasattr(lib, f) and f in host.SYMBOLS, f


def test_invalid_arguments(built_lib):
    lib = host.load_library()
    vp, ci = C.c_void_p, C.c_int
    lib.bnhip_eq_bank_create.argtypes = [ci, ci, C.POINTER(vp)]
    lib.bnhip_eq_bank_add_stream.argtypes = [vp, C.POINTER(ci)]
    lib.bnhip_eq_bank_remove_stream.argtypes = [vp, ci]
    lib.bnhip_eq_bank_set_chain.argtypes = [vp, ci, vp, ci, vp, C.c_double]
    lib.bnhip_eq_bank_reset.argtypes = [vp, ci]
    lib.bnhip_eq_bank_process_pcm16.argtypes = [vp, ci, vp, vp, vp, vp, C.c_size_t, vp]
    lib.bnhip_windows_write_equalized.argtypes = [vp, vp, ci, vp, vp, vp, vp]
    lib.bnhip_eq_bank_destroy.argtypes = [vp]
    lib.bnhip_eq_bank_destroy.restype = None
    design = host._eq_design_fn(lib)
    out = vp()
    assert lib.bnhip_eq_bank_create(0, 4, None) == host.E_INVALID
    assert lib.bnhip_eq_bank_create(0, 0, C.byref(out)) == host.E_INVALID and not out
    s = ci(7)
    assert lib.bnhip_eq_bank_add_stream(None, C.byref(s)) == host.E_INVALID
    assert lib.bnhip_eq_bank_remove_stream(None, 0) == host.E_INVALID
    assert lib.bnhip_eq_bank_reset(None, 0) == host.E_INVALID
    sec = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0])
    one = np.array([1], np.int32)
    assert lib.bnhip_eq_bank_set_chain(None, 0, sec.ctypes.data, 1, one.ctypes.data, 1.0) == host.E_INVALID
    assert lib.bnhip_eq_bank_process_pcm16(None, 0, None, None, None, None, 0, None) == host.E_INVALID
    assert lib.bnhip_windows_write_equalized(None, None, 0, None, None, None, None) == host.E_INVALID
    lib.bnhip_eq_bank_destroy(None)                               # NULL-safe
    o6 = np.zeros(6)
    assert design(0, 48000.0, 1000.0, 0.7, 0.0, 0.0, 1, None) == host.E_INVALID
    assert design(0, 48000.0, 1000.0, 0.7, 0.0, 0.0, 0, o6.ctypes.data) == host.E_INVALID          # passes 0
    assert design(0, 48000.0, 1000.0, 0.0, 0.0, 0.0, 1, o6.ctypes.data) == host.E_INVALID          # q 0: non-finite alpha
    assert design(0, 48000.0, float("nan"), 0.7, 0.0, 0.0, 1, o6.ctypes.data) == host.E_INVALID
    assert design(0, 0.0, 1000.0, 0.7, 0.0, 0.0, 1, o6.ctypes.data) == host.E_INVALID
    assert design(3, 48000.0, 1000.0, 0.0, 0.0, 0.0, 1, o6.ctypes.data) == host.E_INVALID          # BandPass width 0
    assert design(7, 48000.0, 0.0, 0.0, 100.0, 3.0, 1, o6.ctypes.data) == host.E_INVALID          # Peaking frequency 0
    assert design(8, 48000.0, 1000.0, 0.7, 0.0, 0.0, 1, o6.ctypes.data) == host.E_INVALID          # unknown type
    assert design(-1, 48000.0, 1000.0, 0.7, 0.0, 0.0, 1, o6.ctypes.data) == host.E_INVALID
    assert not o6.any()
    with pytest.raises(host.HipError):
        host.design_filter("Notch", 48000, 1000, q=1)


@pytest.mark.parametrize("rate", RATES)
def test_design_matches_python_math(built_lib, rate):
    rng = np.random.default_rng(rate)
    for kind in eqref.TYPES:
        for _ in range(25):
            p = _params(kind, rng)
            got = eqref.normalise(host.design_filter(kind, rate, **p))
            want = eqref.normalise(eqref.design(kind, rate, p["frequency"], q=p["q"], width=p["width"], gain=p["gain"]))
            assert np.abs(np.array(got) - np.array(want)).max() <= 1e-14, (kind, p)
    # the stock chain and a width wider than the centre frequency (hzToOctaves clamps the lower edge to 1 Hz)
    for kind, p in (("HighPass", dict(frequency=100, q=0.7)), ("LowPass", dict(frequency=15000, q=0.7)),
                    ("BandPass", dict(frequency=50, width=400)), ("Peaking", dict(frequency=0.5, width=3, gain=6))):
        got = eqref.normalise(host.design_filter(kind, rate, **p))
        want = eqref.normalise(eqref.design(kind, rate, p["frequency"], q=p.get("q", 0), width=p.get("width", 0), gain=p.get("gain", 0)))
        assert np.abs(np.array(got) - np.array(want)).max() <= 1e-14, (kind, p)


def test_build_filter_chain_follows_the_builder(built_lib):
    assert host.build_filter_chain({"enabled": False, "filters": STOCK["filters"]}, 48000) is None      # disabled
    assert host.build_filter_chain({"enabled": True, "filters": []}, 48000) is None                      # no filters
    assert host.build_filter_chain(None, 48000) is None
    chain = host.build_filter_chain(STOCK, 48000)
    assert [p for _, p in chain] == [1, 1]                                                               # passes 0 -> 1
    assert chain[0][0] == host.design_filter("HighPass", 48000, 100, q=0.7)
    mixed = {"enabled": True, "filters": [{"type": "Unknown", "frequency": 100}, {"type": "LowPass", "frequency": 3000, "q": 1, "passes": 3},
                                          {"type": "BandPass", "frequency": 1000, "width": 0},          # fails validation: skipped
                                          {"type": "Peaking", "frequency": 2000, "width": 500, "gain": 4, "passes": -2}]}
    chain = host.build_filter_chain(mixed, 44100)
    assert [p for _, p in chain] == [3, 1]
    assert chain[1][0] == host.design_filter("Peaking", 44100, 2000, width=500, gain=4)
    assert host.build_filter_chain({"enabled": True, "filters": [{"type": "Unknown"}, {"type": "BandReject", "frequency": 1000}]}, 48000) is None
    assert host.gain_linear(6) == 10 ** (6 / 20) and host.gain_linear(0) == 1.0


def test_oracle_known_answers():
    hp = eqref.design("HighPass", 48000, 100, q=0.7)
    st = {0: eqref.Stream([(hp, 2)])}
    out = eqref.process(st, [(0, np.full(48000, 8000, np.int16))])[0]
    assert out[0] > 7000 and (out[-1000:] == 0).all()                         # DC decays to 0 through a high-pass
    loud = {0: eqref.Stream(None, 10 ** (24 / 20))}
    x = (np.sin(np.arange(4800) * 0.05) * 20000).astype(np.int16)
    y = eqref.process(loud, [(0, x)])[0]
    assert y.max() == 32767 and y.min() == -32767                              # clipped at +24 dB: +-32767
    ident = {0: eqref.Stream()}
    x = np.random.default_rng(1).integers(-32768, 32768, 1000).astype(np.int16)
    assert (eqref.process(ident, [(0, x)])[0] == x).all()                       # gain 1, no chain: the bytes as they are
    # any processing round-trips through float64: -32768 cannot come back (int16(-1 * 32767)), and 32767 loses an LSB
    flat = {0: eqref.Stream(None, 1.0 + 1e-12)}
    assert eqref.process(flat, [(0, np.array([-32768, 32767, 3], np.int16))])[0].tolist() == [-32767, 32766, 2]


def test_equalized_batcher_settings_are_validated():
    from birdnet_go_amd import results as R
    wb = S.WindowBatcher(S.Orchestrator(), R.ResultsQueue(size=10), native=False)
    with pytest.raises(S.StreamError):
        wb.set_processing("a", 0, STOCK)
    wb.set_processing("a", 48000, None, 0.0)                                   # nothing to do: no bank, no stream
    wb.set_processing("a", 48000, {"enabled": False, "filters": STOCK["filters"]})
    assert wb.eq_bank is None and not wb.eq_streams
    wb.close()


# ------------------------------------------------------------------------------------------------ GPU
def _random_chain(rng, rate):
    n = int(rng.integers(0, 9))
    chain, stages = [], 0
    for _ in range(n):
        kind = eqref.TYPES[int(rng.integers(0, 8))]
        passes = int(rng.integers(1, 5))
        if stages + passes > 16:
            break
        p = _params(kind, rng)
        chain.append((host.design_filter(kind, rate, **p), passes))
        stages += passes
    return chain


def _frames(rng, n_streams, per_stream, max_len=3000):
    items = []
    for s in range(n_streams):
        for _ in range(per_stream):
            r = rng.random()
            n = 0 if r < 0.05 else 1 if r < 0.1 else int(rng.integers(2, max_len))
            t = np.arange(n)
            x = 12000 * np.sin(2 * np.pi * (200 + 37 * s) * t / 48000) + rng.normal(0, 3000, n)
            items.append((s, np.clip(x, -32768, 32767).astype(np.int16)))
    rng.shuffle(items)
    return items


def _bank_and_ref(rng, n_streams, rate=48000):
    bank = host.EqualizerBank(max_streams=n_streams)
    ref = {}
    for s in range(n_streams):
        assert bank.add_stream() == s
        kind = s % 8
        if kind == 0:
            chain, gain = [], 1.0                                  # pass-through
        elif kind == 1:
            chain, gain = [], host.gain_linear(float(rng.uniform(-12, 24)))   # gain only
        else:
            chain, gain = _random_chain(rng, rate), host.gain_linear(float(rng.uniform(-12, 24)))
        bank.set_chain(s, chain, gain)
        ref[s] = eqref.Stream(chain, gain)
    return bank, ref


def _check_bytes(got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w.tobytes(), (k, len(g), w.size)


@pytest.mark.gpu
def test_256_streams_byte_identical_to_the_oracle(gpu):
    rng = np.random.default_rng(2024)
    bank, ref = _bank_and_ref(rng, 256)
    for call in range(3):                                          # state carries over calls
        items = _frames(rng, 256, 3)
        _check_bytes(bank.process(items), eqref.process(ref, items))
    # pass-through streams are not converted: -32768 survives
    x = np.array([-32768, 32767, 0, 5], np.int16)
    assert bank.process([(0, x), (8, x)]) == [x.tobytes(), x.tobytes()]
    bank.close()


@pytest.mark.gpu
def test_split_into_other_frames_gives_the_same_bytes(gpu):
    rng = np.random.default_rng(5)
    chain = [(host.design_filter("HighPass", 48000, 100, q=0.7), 2), (host.design_filter("Peaking", 48000, 3000, width=800, gain=9), 3)]
    x = (rng.normal(0, 6000, 20000)).astype(np.int16)
    whole = None
    for cuts in ([], [1, 2, 4800, 9601], [7, 7, 19999], list(range(0, 20000, 1111))):
        bank = host.EqualizerBank(4)
        st = bank.add_stream()
        bank.set_chain(st, chain, host.gain_linear(6))
        edges = [0] + sorted(cuts) + [20000]
        got = b""
        for k, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
            mid = (lo + hi) // 2
            frames = [(st, x[lo:hi])] if k % 2 else [(st, x[lo:mid]), (st, x[mid:hi])]    # several frames of a stream per call too
            got += b"".join(bank.process(frames))
        bank.close()
        whole = whole or got
        assert got == whole
    assert whole == eqref.process({0: eqref.Stream(chain, host.gain_linear(6))}, [(0, x)])[0].tobytes()


@pytest.mark.gpu
def test_set_chain_reset_and_reuse_start_from_zero_state(gpu):
    rng = np.random.default_rng(9)
    a = [(host.design_filter("LowPass", 48000, 2000, q=0.9), 2)]
    b = [(host.design_filter("HighShelf", 48000, 4000, q=0.7, gain=-6), 1), (host.design_filter("AllPass", 48000, 500, q=1.2), 1)]
    x = [rng.normal(0, 8000, 3000).astype(np.int16) for _ in range(4)]
    bank = host.EqualizerBank(4)
    s0, s1 = bank.add_stream(), bank.add_stream()
    bank.set_chain(s0, a, 2.0)
    bank.set_chain(s1, a, 2.0)
    bank.process([(s0, x[0]), (s1, x[0])])
    bank.set_chain(s0, b, 0.5)                                      # new chain, zero state
    bank.reset(s1)                                                  # same chain, zero state
    got = bank.process([(s0, x[1]), (s1, x[1])])
    assert got[0] == eqref.process({0: eqref.Stream(b, 0.5)}, [(0, x[1])])[0].tobytes()
    assert got[1] == eqref.process({0: eqref.Stream(a, 2.0)}, [(0, x[1])])[0].tobytes()
    bank.remove_stream(s1)
    assert bank.add_stream() == s1                                  # the slot is reused with no chain and zero state
    assert bank.process([(s1, x[2])]) == [x[2].tobytes()]
    bank.set_chain(s1, a, 2.0)
    assert bank.process([(s1, x[3])]) == [eqref.process({0: eqref.Stream(a, 2.0)}, [(0, x[3])])[0].tobytes()]
    bank.close()


@pytest.mark.gpu
def test_errors_change_nothing(gpu):
    rng = np.random.default_rng(11)
    chain = [(host.design_filter("BandPass", 48000, 1500, width=600), 2), (host.design_filter("LowShelf", 48000, 300, q=0.8, gain=5), 1)]
    bank = host.EqualizerBank(8)
    st = [bank.add_stream() for _ in range(3)]
    ref = {s: eqref.Stream(chain, 1.5) for s in st}
    for s in st:
        bank.set_chain(s, chain, 1.5)
    gone = bank.add_stream()
    bank.remove_stream(gone)
    warm = [(s, rng.normal(0, 5000, 1000).astype(np.int16)) for s in st]
    _check_bytes(bank.process(warm), eqref.process(ref, warm))
    items = [(s, rng.normal(0, 5000, 700).astype(np.int16)) for s in st] + [(st[0], rng.normal(0, 5000, 300).astype(np.int16))]
    for bad in ([(gone, items[0][1])], [(99, items[0][1])], [(st[1], b"\x01\x02\x03")]):
        with pytest.raises(host.HipError) as e:
            bank.process(items + bad)
        assert e.value.code == host.E_INVALID
    with pytest.raises(host.HipError) as e:
        bank.process(items, out_cap=sum(a.size for _, a in items) - 1)
    assert e.value.code == host.E_INVALID
    # refused chains leave the old chain and its state
    big = [(host.design_filter("LowPass", 48000, 5000, q=0.7), 9), (host.design_filter("HighPass", 48000, 50, q=0.7), 8)]
    with pytest.raises(host.HipError) as e:
        bank.set_chain(st[0], big, 1.0)
    assert e.value.code == host.E_UNSUPPORTED
    for bad in ([((float("nan"), 0, 0, 1, 0, 0), 1)], [((1, 0, 0, 0.0, 0, 0), 1)], [((1, 0, 0, 1, 0, 0), 0)]):
        with pytest.raises(host.HipError) as e:
            bank.set_chain(st[1], bad, 1.0)
        assert e.value.code == host.E_INVALID
    with pytest.raises(host.HipError):
        bank.set_chain(st[2], chain, float("inf"))
    # windows: a removed stream among valid frames fails the whole call, no stream advanced and no ring written
    w = S.NativeWindows(64, 64, max_batch=4)
    srcs = [w.add_source(f"src{k}", 4096) for k in range(3)]
    w.write(srcs[1], b"\x00\x01" * 50)
    before = [w.stats(x) for x in srcs]
    with pytest.raises(S.StreamError):
        bank.write_windows(w, [(s, x, a) for (s, a), x in zip(items, srcs)] + [(gone, srcs[0], items[0][1])])
    assert [w.stats(x) for x in srcs] == before
    w.close()
    _check_bytes(bank.process(items), eqref.process(ref, items))    # exactly the bytes the call would have given
    bank.close()


@pytest.mark.gpu
def test_write_equalized_fills_the_rings_as_process_then_write(gpu):
    rng = np.random.default_rng(13)
    chain = [(host.design_filter("HighPass", 48000, 100, q=0.7), 1), (host.design_filter("LowPass", 48000, 15000, q=0.7), 1)]
    banks, wins = [], []
    for _ in range(2):
        bank = host.EqualizerBank(8)
        win = S.NativeWindows(overlap_bytes=4800, read_bytes=4800)
        for k in range(4):
            s = bank.add_stream()
            win.add_source(f"src{k}", 1 << 16)
            if k:
                bank.set_chain(s, chain if k != 2 else [], host.gain_linear(6) if k != 3 else 1.0)
        banks.append(bank)
        wins.append(win)
    for _ in range(6):
        items = [(k, k, rng.normal(0, 7000, int(rng.integers(0, 3000))).astype(np.int16)) for k in range(4)]
        items += [(1, 1, rng.normal(0, 7000, 500).astype(np.int16))]
        banks[0].write_windows(wins[0], items)
        for (s, src, _), out in zip(items, banks[1].process([(s, f) for s, _, f in items])):
            wins[1].write(src, out)
        a, b = wins[0].collect(), wins[1].collect()
        assert list(a[0]) == list(b[0]) and np.array_equal(np.asarray(a[1]), np.asarray(b[1]))
    with pytest.raises(S.StreamError):
        banks[0].write_windows(wins[0], [(0, 9, np.zeros(10, np.int16))])     # unknown source: nothing runs
    for x in banks + wins:
        x.close()
