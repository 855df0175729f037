"""File analysis of multichannel recordings, the part that needs no device: the restated sample rule (tests/chanref.py) against the
reference's channel policy and against known answers, the new entries' presence, bnhip_analyze_channels_windows against the mixed
table, the length facts of the burst of tests/test_analyze_channels.py (CH_BURST, stated here), and the refusals that are answered
before any device is touched."""
import ctypes as C
import math

import numpy as np
import pytest

from birdnet_go_amd import host

import chanref
from test_analyze_mixed_ref import CLIP, HOP, K, MIN_TAIL, MODEL_RATE, TILE, _bad_tables

ENERGY_TILE = 16384                                       # frames of one block of k_channel_energy (csrc/channels.h)
# (rate, bits, frames, channels, the channel the fixed-channel test reads): all four depths; 1, 2, 3, 4 and 8 channels; rates at and
# off the model's; a 24-bit 3-channel recording (9-byte frames, no sample aligned); n_out = TILE + 1; an n_out that is no multiple of
# 4; a recording of one frame; a mono one; a long one that brings W above 64
CH_BURST = [(44100, 16, 7526, 2, 1), (96000, 24, 8193, 3, 2), (32000, 32, 16002, 4, 0), (48000, 16, 31001, 8, 5), (250000, 0, 70000, 2, 1),
            (44100, 16, 1, 2, 0), (48000, 24, 9001, 1, 0), (44100, 16, 300000, 2, 0)]
CH_N_OUT = [8192, 4097, 24003, 31001, 13440, 2, 9001, 326531]
CH_FIRST = [0, 1, 2, 5, 10, 12, 13, 14, 68]


def ch_recs(burst=CH_BURST, select=None):
    """The CHANNELS_RECORDING table of a burst; select: one selection for all, or None for each row's own channel."""
    return host.channel_recordings([b[2] for b in burst], [b[0] for b in burst], [b[1] for b in burst], [b[3] for b in burst],
                                   [b[4] for b in burst] if select is None else select)


# ---- the rule
def _stereo(rng, n, a_left, a_right):
    x = np.stack([a_left * rng.standard_normal(n), a_right * rng.standard_normal(n)], axis=1)
    return np.clip(np.round(x), -32768, 32767).astype(np.int64)


def test_decision_is_the_reference_rule():
    """decide() on exact sums, with no logarithm, is recommendChannel(computeRmsDbfs(L), computeRmsDbfs(R)) with math.log10, on a
    seeded sweep of stereo cases: levels from silence to near full scale, leads from 0 to 20 dB either way, kept 0.05 dB away from
    the 6 dB and -60 dBFS lines (where the two forms may differ by the rounding of a logarithm)."""
    rng = np.random.default_rng(2024)
    seen = set()
    n_cases = 0
    while n_cases < 400:
        n = int(rng.integers(50, 2000))
        level = 10.0 ** rng.uniform(-0.5, 4.0)             # rms in 16-bit units: 0.3 .. 10 000
        lead = rng.uniform(-20.0, 20.0)
        f = _stereo(rng, n, level, level * 10.0 ** (-lead / 20.0))
        e = chanref.energies(f)
        db = [chanref.rms_dbfs(v, 16, n) for v in e]
        near = min(abs(abs(db[0] - db[1]) - 6.0), abs(db[0] + 60.0), abs(db[1] + 60.0))
        if near < 0.05:
            continue
        want = chanref.go_rule(f[:, 0], f[:, 1])
        assert chanref.decide(e, 16, n) == want, (n, db)
        seen.add(want)
        n_cases += 1
    assert seen == {0, 1, chanref.MIX}


def test_known_answers():
    n = 4800
    const = np.full((n, 2), 16384, np.int64)
    const[1::2] *= -1
    e = chanref.energies(const)
    assert e == [n * 16384 ** 2] * 2
    assert abs(chanref.rms_dbfs(e[0], 16, n) - 20.0 * math.log10(0.5)) < 1e-12 and abs(chanref.rms_dbfs(e[0], 16, n) + 6.0206) < 1e-4
    # the same level at 24 and 32 bits: the samples shifted up, the dB unchanged
    for bits in (24, 32):
        assert abs(chanref.rms_dbfs(chanref.energies(const << (bits - 16))[0], bits, n) + 6.0206) < 1e-4
    assert chanref.rms_dbfs(0, 16, n) == -96.0
    few = np.zeros((n, 1), np.int64)
    few[::2] = 1                                           # rms = sqrt(1 / 2) < 1
    assert chanref.rms_dbfs(chanref.energies(few)[0], 16, n) == -96.0
    # a lead stated in dB: constant channels of amplitudes a and a * 10^(-lead / 20), exact sums of the rounded amplitudes
    def lead(db_lead, loud=10000.0, swap=False):
        a = [int(round(loud)), int(round(loud * 10.0 ** (-db_lead / 20.0)))]
        a = a[::-1] if swap else a
        f = np.stack([np.full(n, a[0], np.int64), np.full(n, a[1], np.int64)], axis=1)
        return chanref.decide(chanref.energies(f), 16, n)
    assert lead(6.1) == 0 and lead(6.1, swap=True) == 1
    assert lead(5.9) == chanref.MIX and lead(5.9, swap=True) == chanref.MIX
    # both at -61 dBFS (29.2 of 32768; the line is 32.768): mix, even with one of them 20 dB down; one at -59 and a lead: picked
    q = 32768.0 * 10.0 ** (-61.0 / 20.0)
    assert lead(0.0, loud=q) == chanref.MIX and lead(20.0, loud=q) == chanref.MIX
    assert lead(20.0, loud=32768.0 * 10.0 ** (-59.0 / 20.0)) == 0
    # ties go to the lower index; one channel is channel 0, silent or not; four channels
    assert chanref.decide([100 * n * 4000, 100 * n * 4000, 7], 16, n) == chanref.MIX
    assert chanref.decide([0], 16, n) == 0
    assert chanref.decide([5 * n * 10 ** 6, 6 * n * 10 ** 6, 100 * n * 10 ** 6, 7 * n * 10 ** 6], 16, n) == 2
    # the line scales with the depth: the same recording shifted up decides the same
    f = np.stack([np.full(n, 30, np.int64), np.full(n, 3, np.int64)], axis=1)
    assert chanref.decide(chanref.energies(f), 16, n) == chanref.MIX
    assert chanref.decide(chanref.energies(f << 16), 32, n) == chanref.MIX
    assert chanref.decide(chanref.energies(f * 2), 16, n) == 0
    # the mix: integer depths divide the exact sum once; float32 adds in fp64
    f3 = np.array([[32767, 32767, 32766], [-32768, -32768, -32768], [1, 0, 0]], np.int64)
    assert chanref.mix(f3, 16).tolist() == [np.float32(98300 / 98304), -1.0, np.float32(1 / 98304)]
    ff = np.array([[1.0, 2.0 ** -30, -1.0]], np.float32)
    assert chanref.mix(ff, 0).tolist() == [np.float32(2.0 ** -30 / 3.0)]        # (float32 accumulation would lose the small one)


# ---- the entries
def test_symbols_exported_and_prototyped(built_lib):
    lib = host.load_library()
    names = ["bnhip_analyze_channels_windows", "bnhip_analyze_channels_pcm_topk", "bnhip_analyze_channels_pcm", "bnhip_channel_energy_pcm"]
    for name in names:
        assert name in host.SYMBOLS and hasattr(lib, name), name
    host._analyze_channels_protos(lib)
    assert len(lib.bnhip_analyze_channels_pcm_topk.argtypes) == len(lib.bnhip_analyze_mixed_pcm_topk.argtypes) + 1
    assert len(lib.bnhip_analyze_channels_pcm.argtypes) == len(lib.bnhip_analyze_mixed_pcm.argtypes) + 1
    assert host.CHANNELS_RECORDING.itemsize == 24 and host.CHANNEL_ENERGY.itemsize == 24
    assert (host.CHANNEL_MIX, host.CHANNEL_AUTO) == (chanref.MIX, chanref.AUTO) == (-1, -2)
    import os
    header = open(os.path.join(os.path.dirname(host.__file__), "..", "include", "bnhip.h")).read()
    for name in names + ["#define BNHIP_CHANNEL_MIX  (-1)", "#define BNHIP_CHANNEL_AUTO (-2)", "bnhip_channels_recording", "bnhip_channel_energy"]:
        assert name in header, name


@pytest.mark.parametrize("hop,min_tail", [(HOP, MIN_TAIL), (HOP + 1, 0), (CLIP, CLIP)])
def test_channels_windows_is_the_mixed_table(built_lib, hop, min_tail):
    """The table over (length, rate): the channels and the selection do not enter it."""
    base = host.recordings([b[2] for b in CH_BURST], [b[0] for b in CH_BURST], [b[1] for b in CH_BURST])
    want_first, want_out = host.analyze_mixed_windows(base, MODEL_RATE, CLIP, hop, min_tail)
    for select in (None, "mix", 0):
        first, n_out = host.analyze_channels_windows(ch_recs(select=select), MODEL_RATE, CLIP, hop, min_tail)
        assert first.dtype == np.int64 and np.array_equal(first, want_first) and np.array_equal(n_out, want_out)
    lib = host._analyze_channels_protos(host.load_library())
    recs, out = ch_recs(), np.zeros(len(CH_BURST) + 1, np.int64)
    assert lib.bnhip_analyze_channels_windows(recs.ctypes.data, len(recs), MODEL_RATE, CLIP, hop, min_tail, out.ctypes.data, None) == want_first[-1]
    assert np.array_equal(out, want_first)


def test_burst_facts(built_lib):
    """(CPU) what the burst of the GPU tests is there for."""
    first, n_out = host.analyze_channels_windows(ch_recs(), MODEL_RATE, CLIP, HOP, MIN_TAIL)
    assert n_out.tolist() == CH_N_OUT and first.tolist() == CH_FIRST
    assert {b[1] for b in CH_BURST} == {0, 16, 24, 32} and {b[3] for b in CH_BURST} == {1, 2, 3, 4, 8}
    assert any(b[0] == MODEL_RATE and b[3] > 1 for b in CH_BURST) and any(b[0] != MODEL_RATE and b[3] > 1 for b in CH_BURST)
    assert (CH_BURST[1][1], CH_BURST[1][3]) == (24, 3) and CH_N_OUT[1] == TILE + 1          # 9-byte frames, one output past a tile
    assert CH_N_OUT[2] % 4 == 3 and CH_BURST[5][2] == 1
    assert all(0 <= b[4] < b[3] for b in CH_BURST) and any(b[4] == b[3] - 1 > 0 for b in CH_BURST) and any(b[4] == 0 for b in CH_BURST)
    W = CH_FIRST[-1]
    assert W > 64 and W % 32 <= 16 and CH_FIRST[7] < 32                                     # three chunks, the first straddling all eight


def _bad_channel_tables():
    """(what is wrong, CHANNELS_RECORDING table): every refusal the channels add to the mixed call's."""
    ok = [(44100, 16, 7526, 2, 1), (48000, 24, 100, 3, 0)]
    big = (1 << 31) - 1
    return [("no channel", ch_recs(ok + [(48000, 16, 10, 0, 0)])), ("17 channels", ch_recs([(48000, 16, 10, 17, 0)] + ok)),
            ("negative channels", ch_recs(ok + [(48000, 16, 10, -2, 0)])),
            ("select = channels", ch_recs(ok + [(48000, 16, 10, 2, 2)])), ("select -3", ch_recs(ok + [(48000, 16, 10, 2, -3)])),
            ("select 1 of a mono recording", ch_recs(ok + [(48000, 16, 10, 1, 1)])),
            ("auto on float32", ch_recs(ok + [(48000, 0, 10, 2, chanref.AUTO)])), ("auto on mono float32", ch_recs([(48000, 0, 10, 1, chanref.AUTO)])),
            ("2^36 samples in 3 * 2^31 frames", ch_recs([(48000, 16, big, 16, 0)] * 3))]


def test_windows_refusals(built_lib):
    lib = host._analyze_channels_protos(host.load_library())
    f = lib.bnhip_analyze_channels_windows
    first, n_out = np.full(16, -7, np.int64), np.full(16, -7, np.int64)
    P = lambda a: a.ctypes.data
    for what, bad in _bad_channel_tables():
        assert f(P(bad), len(bad), MODEL_RATE, CLIP, HOP, 0, P(first), P(n_out)) == host.E_INVALID, what
    for what, bad, rate in _bad_tables():                  # everything the mixed table refuses, as stereo
        tab = host.channel_recordings(bad["length"], bad["rate"], bad["bits_per_sample"], 2, 0)
        assert f(P(tab), len(tab), rate, CLIP, HOP, 0, P(first), P(n_out)) == host.E_INVALID, what
    recs = ch_recs()
    for args in [(None, 8, MODEL_RATE, CLIP, HOP, 0), (P(recs), 0, MODEL_RATE, CLIP, HOP, 0), (P(recs), 65536, MODEL_RATE, CLIP, HOP, 0),
                 (P(recs), 8, MODEL_RATE, CLIP, 0, 0), (P(recs), 8, MODEL_RATE, CLIP, CLIP + 1, 0), (P(recs), 8, MODEL_RATE, CLIP, HOP, -1)]:
        assert f(*args, P(first), P(n_out)) == host.E_INVALID, args
    assert f(P(recs), 8, MODEL_RATE, CLIP, HOP, 0, None, P(n_out)) == host.E_INVALID
    assert (first == -7).all() and (n_out == -7).all()
    # 2^36 - 1 samples are no refusal (2 * 16 * (2^31 - 1) + 31), one more is
    most = [(48000, 16, (1 << 31) - 1, 16, 0)] * 2
    assert host.analyze_channels_windows(ch_recs(most + [(48000, 16, 31, 1, 0)]), MODEL_RATE, 144000, 144000)[0][-1] == 2 * 14914 + 1
    with pytest.raises(host.HipError) as ei:
        host.analyze_channels_windows(ch_recs(most + [(48000, 16, 32, 1, 0)]), MODEL_RATE, 144000, 144000)
    assert ei.value.code == host.E_INVALID and "2^36" in str(ei.value)


def test_device_entries_refuse_before_the_device(built_lib, tiny_blob):
    """bnhip_analyze_channels_pcm_topk / bnhip_analyze_channels_pcm on a plan-only handle: a well-formed call is refused for the handle
    ("plan-only"), every bad table for the table, with nothing written; bnhip_channel_energy_pcm answers its argument errors before it
    looks for a device."""
    lib = host._analyze_channels_protos(host.load_library())
    m = host.HipClassifier(tiny_blob, plan_only=True)
    P = lambda a: a.ctypes.data
    try:
        n = m.n_samples
        good = host.channel_recordings([2 * n, n + 5], [44100, 48000], [16, 24], [2, 3], ["auto", "mix"])
        pcm = np.zeros(2 * n * 2 * 2 + (n + 5) * 3 * 3, np.uint8)
        conf, idx = np.full((8, 5), -7, np.float32), np.full((8, 5), -7, np.int32)
        rows = np.zeros(40, host.DETECTION)
        rows["window"] = -7
        n_out, chosen = C.c_size_t(12345), np.full(16, -7, np.int32)
        topk = lambda rc=good, rate=MODEL_RATE: lib.bnhip_analyze_channels_pcm_topk(m._h, P(pcm), P(rc), len(rc), rate, n // 2, 0, 0, 1.0, 5, P(conf),
                                                                                   P(idx), P(chosen))
        det = lambda rc=good, rate=MODEL_RATE: lib.bnhip_analyze_channels_pcm(m._h, P(pcm), P(rc), len(rc), rate, n // 2, 0, 0, 1.0, 5, 0.0, P(rows), 40,
                                                                             C.byref(n_out), P(chosen))
        for f in (topk, det):
            assert f() == host.E_INVALID and b"plan-only" in lib.bnhip_last_error()
            for what, bad in _bad_channel_tables():
                assert f(rc=bad) == host.E_INVALID, what
                assert b"plan-only" not in lib.bnhip_last_error(), what
            for what, bad, rate in _bad_tables():
                tab = host.channel_recordings(bad["length"], bad["rate"], bad["bits_per_sample"], 2, "mix")
                assert f(rc=tab, rate=rate) == host.E_INVALID, what
                assert b"plan-only" not in lib.bnhip_last_error(), what
        assert lib.bnhip_analyze_channels_pcm_topk(m._h, P(pcm), P(good), 2, MODEL_RATE, n // 2, 0, 0, 1.0, 5, P(conf), P(idx), None) == host.E_INVALID
        assert b"plan-only" in lib.bnhip_last_error()                      # (chosen may be NULL: refused for the handle alone)
        with pytest.raises(host.HipError):
            m.analyze_channels_pcm_topk(pcm[:-1].tobytes(), good, MODEL_RATE, n // 2)      # the bytes do not match the frames
        energy = np.zeros(64, host.CHANNEL_ENERGY)
        energy["rms_dbfs"] = -7.0
        e = lambda x=P(pcm), rc=good, nr=None, o=P(energy): lib.bnhip_channel_energy_pcm(0, x, None if rc is None else P(rc),
                                                                                         len(rc) if nr is None else nr, o, P(chosen))
        for what, bad in _bad_channel_tables():
            assert e(rc=bad) == host.E_INVALID, what
        for bad in [ch_recs([(48000, 0, 10, 2, 0)]), ch_recs([(48000, 8, 10, 2, 0)]), ch_recs([(0, 16, 10, 2, 0)]), ch_recs([(48000, 16, 0, 2, 0)]),
                    ch_recs([(48000, 16, 1 << 31, 2, 0)])]:
            assert e(rc=bad) == host.E_INVALID, bad
        assert e(x=None) == host.E_INVALID and e(rc=None, nr=2) == host.E_INVALID and e(o=None) == host.E_INVALID
        assert e(nr=0) == host.E_INVALID and e(nr=65536) == host.E_INVALID
        assert (conf == -7).all() and (idx == -7).all() and (rows["window"] == -7).all() and n_out.value == 12345
        assert (chosen == -7).all() and (energy["rms_dbfs"] == -7.0).all()
        assert m.describe()["n_samples"] == n
    finally:
        m.close()
    multi = host.HipClassifier(tiny_blob, plan_only=True, devices=[0, 0])
    try:
        assert lib.bnhip_analyze_channels_pcm_topk(multi._h, P(pcm), P(good), 2, MODEL_RATE, n // 2, 0, 0, 1.0, 5, P(conf), P(idx), P(chosen)) == host.E_INVALID
        assert b"single-device" in lib.bnhip_last_error()
    finally:
        multi.close()
