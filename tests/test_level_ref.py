"""The audio level rule without a device: known answers, the host-only entry bnhip_audio_level against the restatement
(tests/levelref.py), the summary's derived fields, and the new names in the C ABI."""
import ctypes as C
import math

import numpy as np
import pytest

from birdnet_go_amd import host

import levelref

ENTRIES = ("bnhip_audio_level", "bnhip_level_bank_create", "bnhip_level_bank_add_stream", "bnhip_level_bank_remove_stream",
           "bnhip_level_bank_process_pcm", "bnhip_level_bank_latest", "bnhip_level_bank_stats", "bnhip_level_bank_reset",
           "bnhip_level_bank_destroy", "bnhip_capture_bank_write_levels")

# a frame of constant amplitude a -> (level, clipping); computed from the rule (a = 1036: 59.996, a = 1037: 60.013,
# a = 5826: 89.9968, a = 5827: 89.9998)
KNOWN = [(0, 0, False), (33, 0, False), (184, 29, False), (185, 30, False), (1036, 59, False), (1037, 60, False), (5826, 89, False),
         (5827, 89, False), (32767, 100, True), (-32768, 100, True)]


@pytest.mark.parametrize("a,level,clipping", KNOWN)
def test_known_answers(built_lib, a, level, clipping):
    n = 480
    total, clipped, lv, cl = levelref.measure(np.full(n, a, np.int16))
    assert total == n * a * a and (lv, cl) == (level, clipping) and clipped == (n if clipping else 0)
    assert host.audio_level(total, n, cl) == level


def test_single_full_scale_sample_and_empty_frame(built_lib):
    q = np.full(4800, 3, np.int16)
    q[1234] = 32767
    total, clipped, lv, cl = levelref.measure(q)
    assert (clipped, lv, cl) == (1, 95, True) and levelref.level(total, q.size, False) < 95
    assert host.audio_level(total, q.size, True) == 95
    assert levelref.measure(np.zeros(0, np.int16)) == (0, 0, 0, False)
    assert host.audio_level(0, 0, False) == 0 and host.audio_level(0, 0, True) == 0
    assert host.audio_level(0, 100, False) == 0                       # silence: log10(0) = -Inf, clamped


def test_entry_equals_the_restatement_over_a_sweep(built_lib):
    """(sum, n, clipping) triples whose scaled value lies at least 1e-9 from every integer - a condition on the inputs that the
    restatement alone decides, asserted on its values first - give the same level from the library's sqrt and log10."""
    rng = np.random.default_rng(20)
    triples = []
    while len(triples) < 4000:
        n = int(rng.integers(1, levelref.MAX_FRAME + 1)) if rng.random() < 0.5 else int(rng.integers(1, 5000))
        amp = float(10 ** rng.uniform(0, math.log10(32768.0)))           # an RMS between 1 and full scale
        s = min(int(amp * amp * n * rng.uniform(0.5, 1.5)), n << 30)
        clip = bool(rng.random() < 0.3)
        v = levelref.scaled(s, n, clip) if s else -math.inf
        if s and abs(v - round(v)) < 1e-9:
            continue
        triples.append((s, n, clip))
    for s, n, clip in triples:
        v = levelref.scaled(s, n, clip) if s else -math.inf
        assert not s or abs(v - round(v)) >= 1e-9
    assert len({levelref.level(*t) for t in triples}) > 90              # the sweep covers the scale
    for t in triples:
        assert host.audio_level(*t) == levelref.level(*t), t


def test_entry_refusals(built_lib):
    lib = host.load_library()
    lib.bnhip_audio_level.argtypes = [C.c_uint64, C.c_int64, C.c_int, C.POINTER(C.c_int)]
    lv = C.c_int(7)
    assert lib.bnhip_audio_level(1, 1, 0, None) == host.E_INVALID
    assert lib.bnhip_audio_level(1, -1, 0, C.byref(lv)) == host.E_INVALID
    assert lib.bnhip_audio_level(1, levelref.MAX_FRAME + 1, 0, C.byref(lv)) == host.E_INVALID
    assert lib.bnhip_audio_level(levelref.MAX_FRAME << 30, levelref.MAX_FRAME, 1, C.byref(lv)) == host.BNHIP_OK and lv.value == 100


def test_stats_fields_over_a_random_sequence():
    rng = np.random.default_rng(21)
    st = levelref.Stats()
    assert st.fields() == dict(sum=0, count=0, zero_count=0, clip_count=0, min=0, max=0, avg_level=0, zero_pct=0, clipping_pct=0)
    levels = [int(v) for v in rng.integers(0, 101, 300)]
    for i in range(0, 300, 7):
        levels[i] = 0
    clips = [bool(v) for v in rng.random(300) < 0.1]
    for lv, cl in zip(levels, clips):
        st.record(lv, cl)
    f = st.fields()
    assert f["count"] == 300 and f["sum"] == sum(levels) and f["min"] == 0 and f["max"] == max(levels)
    assert f["zero_count"] == levels.count(0) >= 43 and f["clip_count"] == sum(clips) > 0
    assert f["avg_level"] == sum(levels) // 300 and f["zero_pct"] == levels.count(0) * 100 // 300 and f["clipping_pct"] == sum(clips) * 100 // 300


def test_symbols_and_record_sizes(built_lib):
    lib = C.CDLL(built_lib)
    for s in ENTRIES:
        assert s in host.SYMBOLS and hasattr(lib, s), s
    assert host.AUDIO_LEVEL.itemsize == 40 and host.AUDIO_LEVEL_STATS.itemsize == 56


def test_level_bank_refusals_without_a_device(built_lib):
    lib = host.load_library()
    vp, ci = C.c_void_p, C.c_int
    lib.bnhip_level_bank_create.argtypes = [ci, ci, C.POINTER(vp)]
    h = vp()
    assert lib.bnhip_level_bank_create(0, 1, None) == host.E_INVALID
    for bad in (0, -1, 65536):
        assert lib.bnhip_level_bank_create(0, bad, C.byref(h)) == host.E_INVALID and not h
    lib.bnhip_level_bank_destroy.argtypes = [vp]
    lib.bnhip_level_bank_destroy.restype = None
    lib.bnhip_level_bank_destroy(None)
