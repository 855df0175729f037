"""The sound level bank (bnhip_soundlevel_*): the 1/3-octave sound level monitor (soundlevel.Processor,
internal/audiocore/soundlevel/processor.go) for many sources in one device call per call, report for report against the
float64 restatement in tests/slref.py; the band designer against Python's math; the Go shim's surface and its restated report
struct against the header."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import slref
from birdnet_go_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPDIR = os.path.join(ROOT, "birdnet-go_amd", "go", "internal", "inference", "hip")
ENTRIES = ("bnhip_soundlevel_bands", "bnhip_soundlevel_bank_create", "bnhip_soundlevel_bank_add_stream",
           "bnhip_soundlevel_bank_remove_stream", "bnhip_soundlevel_bank_reset", "bnhip_soundlevel_bank_process_pcm16",
           "bnhip_soundlevel_bank_destroy")
COUNTS = {8000: 22, 16000: 25, 22050: 26, 32000: 28, 44100: 29, 48000: 30, 96000: 30, 256000: 30}


def _lib():
    lib = host.load_library()
    vp, ci = C.c_void_p, C.c_int
    lib.bnhip_soundlevel_bands.argtypes = [ci, vp, ci, vp]
    lib.bnhip_soundlevel_bank_create.argtypes = [ci, ci, ci, vp, ci, C.POINTER(vp)]
    lib.bnhip_soundlevel_bank_add_stream.argtypes = [vp, ci, vp]
    lib.bnhip_soundlevel_bank_remove_stream.argtypes = [vp, ci]
    lib.bnhip_soundlevel_bank_reset.argtypes = [vp, ci]
    lib.bnhip_soundlevel_bank_process_pcm16.argtypes = [vp, ci, vp, vp, vp, vp, ci, vp]
    lib.bnhip_soundlevel_bank_destroy.argtypes = [vp]
    lib.bnhip_soundlevel_bank_destroy.restype = None
    return lib


# ------------------------------------------------------------------------------------------------ CPU
def test_symbols_exported_and_listed(built_lib):
    lib = C.CDLL(built_lib)
    for f in ENTRIES:
        assert hasattr(lib, f) and f in host.SYMBOLS, f


def test_invalid_arguments(built_lib):
    lib = _lib()
    out, n = C.c_void_p(), C.c_int(7)
    tbl = np.array(slref.design(48000), np.float64)
    assert lib.bnhip_soundlevel_bank_create(0, 48000, 4, None, 0, None) == host.E_INVALID
    assert lib.bnhip_soundlevel_bank_create(0, 0, 4, None, 0, C.byref(out)) == host.E_INVALID and not out      # fs <= 0
    assert lib.bnhip_soundlevel_bank_create(0, -8000, 4, None, 0, C.byref(out)) == host.E_INVALID and not out
    assert lib.bnhip_soundlevel_bank_create(0, 48000, 0, None, 0, C.byref(out)) == host.E_INVALID and not out  # max_streams
    assert lib.bnhip_soundlevel_bank_create(0, 48000, 4, tbl.ctypes.data, 0, C.byref(out)) == host.E_INVALID and not out
    assert lib.bnhip_soundlevel_bank_create(0, 48000, 4, tbl.ctypes.data, 33, C.byref(out)) == host.E_INVALID and not out
    assert lib.bnhip_soundlevel_bank_add_stream(None, 10, C.byref(n)) == host.E_INVALID
    assert lib.bnhip_soundlevel_bank_remove_stream(None, 0) == host.E_INVALID
    assert lib.bnhip_soundlevel_bank_reset(None, 0) == host.E_INVALID
    assert lib.bnhip_soundlevel_bank_process_pcm16(None, 0, None, None, None, None, 0, C.byref(n)) == host.E_INVALID
    lib.bnhip_soundlevel_bank_destroy(None)                                     # NULL-safe
    assert lib.bnhip_soundlevel_bands(48000, None, 0, None) == host.E_INVALID
    assert lib.bnhip_soundlevel_bands(0, None, 0, C.byref(n)) == host.E_INVALID and n.value == 0
    assert lib.bnhip_soundlevel_bands(48000, None, 0, C.byref(n)) == host.BNHIP_OK and n.value == 30   # the count only
    small = np.zeros((29, 6))
    assert lib.bnhip_soundlevel_bands(48000, small.ctypes.data, 29, C.byref(n)) == host.E_INVALID and not small.any()
    with pytest.raises(host.HipError):
        host.sound_level_bands(-1)


@pytest.mark.parametrize("rate", sorted(COUNTS))
def test_bands_match_the_restatement(built_lib, rate):
    got, want = host.sound_level_bands(rate), slref.design(rate)
    assert len(got) == COUNTS[rate] == len(want)
    assert got == want                                                          # bit for bit: both use the C library's math
    assert got[0][0] == 25.0 and got[0][2] == 0.0                               # b1 = 0 / a0


def test_caller_tables_are_validated(built_lib):
    lib = _lib()
    good = np.array(slref.design(48000), np.float64)
    out = C.c_void_p()
    bad = []
    for j, v in ((0, float("nan")), (3, float("inf")), (0, 0.0), (0, -25.0)):
        t = good.copy()
        t[1, j] = v
        bad.append(t)
    t = good.copy(); t[2, 5] = 1.0; bad.append(t)                               # |a2| >= 1
    t = good.copy(); t[2, 4] = -(1.0 + t[2, 5]); bad.append(t)                  # |a1| >= 1 + a2
    for t in bad:
        assert lib.bnhip_soundlevel_bank_create(0, 48000, 4, t.ctypes.data, len(t), C.byref(out)) == host.E_INVALID and not out
    with pytest.raises(host.HipError) as e:
        host.SoundLevelBank(48000, bands=bad[-1])
    assert e.value.code == host.E_INVALID


def test_band_keys_follow_format_band_key():
    # processor_test.go:286-308
    for hz, key in ((25, "25.0_Hz"), (31.5, "31.5_Hz"), (999.9, "999.9_Hz"), (1000, "1.0_kHz"), (1000.0, "1.0_kHz"),
                    (12500, "12.5_kHz"), (20000, "20.0_kHz")):
        assert host.sound_level_band_key(hz) == key == slref.band_key(hz)


def test_restatements_agree(built_lib):
    """The numpy and the C restatement give the same reports (re-framed, several streams, a silence tail through subnormals)."""
    rng = np.random.default_rng(5)
    frames = [(k % 3, rng.integers(-32768, 32768, int(rng.integers(0, 7000))).astype(np.int16)) for k in range(14)]
    frames += [(0, np.zeros(9000, np.int16))]
    a = {k: slref.Processor(8000, 1 + k // 2) for k in range(3)}
    b = {k: slref.Processor(8000, 1 + k // 2) for k in range(3)}
    ra, rb = slref.process(a, frames, native=False), slref.process(b, frames, native=True)
    assert len(ra) >= 4 and ra == rb


def test_kernel_has_no_fused_multiply_add(built_lib):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_audit
    if not os.path.exists(isa_audit.OBJDUMP):
        pytest.skip("llvm-objdump not found")
    import tempfile
    ops = []
    for _, blob in isa_audit.code_objects(built_lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob); f.flush()
            txt = subprocess.run([isa_audit.OBJDUMP, "-d", "--no-show-raw-insn", f.name], capture_output=True, text=True, check=True).stdout
        if "k_soundlevel_bank" not in txt:
            continue
        body = txt[txt.index("k_soundlevel_bank"):]
        body = body[body.index(">:") + 2:]
        body = body[:body.find(">:")] if ">:" in body else body
        ops += re.findall(r"^\s+(v_\w+)", body, flags=re.M)
    assert ops.count("v_mul_f64") >= 6 * 32 and "v_add_f64" in ops                # the unrolled recurrence really was read
    assert not [o for o in ops if "fma" in o or "mac" in o], sorted({o for o in ops if "fma" in o or "mac" in o})


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present")
def test_bank_without_device_is_a_loud_error(built_lib):
    lib = _lib()
    h = C.c_void_p()
    assert lib.bnhip_soundlevel_bank_create(0, 48000, 8, None, 0, C.byref(h)) == host.E_NO_DEVICE and not h.value
    with pytest.raises(host.ErrHIPUnavailable):
        host.SoundLevelBank(48000)


# ------------------------------------------------------------------------------------------------ Go shim (CPU)
def test_go_shim_carries_the_sound_level_surface():
    src = open(os.path.join(HIPDIR, "backend_hip.go")).read()
    stub = open(os.path.join(HIPDIR, "stub_nohip.go")).read()
    for sig in ("func NewSoundLevelBank(sampleRate, maxStreams, device int, bands []SoundLevelBand) (*SoundLevelBank, error)",
                "func (b *SoundLevelBank) AddStream(intervalSeconds int) (int, error)",
                "func (b *SoundLevelBank) RemoveStream(stream int) error",
                "func (b *SoundLevelBank) Reset(stream int) error",
                "func (b *SoundLevelBank) Process(streams []int, frames [][]byte) ([]SoundLevelReport, error)",
                "func (b *SoundLevelBank) Close() error"):
        assert sig in src, sig
    for sig in ("func NewSoundLevelBank(int, int, int, []SoundLevelBand) (*SoundLevelBank, error)",
                "func (*SoundLevelBank) AddStream(int) (int, error)", "func (*SoundLevelBank) RemoveStream(int) error",
                "func (*SoundLevelBank) Reset(int) error", "func (*SoundLevelBank) Process([]int, [][]byte) ([]SoundLevelReport, error)",
                "func (*SoundLevelBank) Close() error"):
        assert sig in stub, sig
    pure = open(os.path.join(HIPDIR, "soundlevel.go")).read()
    assert "//go:build" not in pure.split("package hip")[0]                    # built with and without the hip tag
    assert "func BuildSoundLevelBands(sampleRate int) ([]SoundLevelBand, error)" in pure
    assert "func SoundLevelBandKey(centerFreq float64) string" in pure
    for fn in ("func NewSoundLevelBank(", "func (b *SoundLevelBank) AddStream(", "func (b *SoundLevelBank) RemoveStream(",
               "func (b *SoundLevelBank) Reset(", "func (b *SoundLevelBank) Process("):
        body = src[src.index(fn):]
        body = body[:body.index("\n}\n")]
        assert "runtime.LockOSThread()" in body and "defer runtime.UnlockOSThread()" in body, fn
    for name in ("sl_bands", "sl_create", "sl_add_stream", "sl_remove_stream", "sl_reset", "sl_process_pcm16", "sl_destroy"):
        assert f"static inline" in src[src.index(f"bnbind_{name}(") - 40:src.index(f"bnbind_{name}(")], name


LAYOUT_C = r"""
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include HDR
#define F(m) printf(#m " %zu %zu\n", offsetof(bnhip_sound_level, m), sizeof(((bnhip_sound_level*)0)->m))
int main(void) {
    printf("size %zu align %zu\n", sizeof(bnhip_sound_level), _Alignof(bnhip_sound_level));
    F(stream); F(frame); F(duration_s); F(n_bands); F(center_hz); F(min_db); F(max_db); F(mean_db); F(sample_count);
    return 0;
}
"""


def test_go_preamble_restates_the_report_struct(tmp_path):
    """The cgo preamble declares its own bnhip_sound_level: sizeof and every offsetof must be the header's."""
    src = open(os.path.join(HIPDIR, "backend_hip.go")).read()
    m = re.search(r"package hip\s*/\*(.*?)\*/\s*import \"C\"", src, flags=re.S)
    pre = "\n".join(l for l in m.group(1).splitlines() if not l.startswith("#cgo"))
    (tmp_path / "pre.h").write_text(pre)
    (tmp_path / "layout.c").write_text(LAYOUT_C)
    outs = []
    for hdr in (str(tmp_path / "pre.h"), os.path.join(ROOT, "include", "bnhip.h")):
        exe = str(tmp_path / ("a%d" % len(outs)))
        subprocess.check_call(["gcc", "-std=c11", "-D_DEFAULT_SOURCE", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function",
                               f'-DHDR="{hdr}"', str(tmp_path / "layout.c"), "-o", exe, "-ldl"])
        outs.append(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    assert outs[0] == outs[1] and "sample_count" in outs[0], outs


# ------------------------------------------------------------------------------------------------ GPU
def _setup(rate, intervals, max_streams=None):
    bank = host.SoundLevelBank(rate, max_streams=max_streams or len(intervals))
    sts = [bank.add_stream(iv) for iv in intervals]
    procs = {s: slref.Processor(rate, iv) for s, iv in zip(sts, intervals)}
    return bank, sts, procs


def _tone(hz, amp, n, rate, phase=0):
    t = (np.arange(n) + phase) / rate
    return np.round(amp * 32767 * np.sin(2 * np.pi * hz * t)).astype(np.int16)


@pytest.mark.gpu
def test_256_streams_match_the_restatement(gpu):
    rng = np.random.default_rng(11)
    bank, sts, procs = _setup(16000, [int(v) for v in rng.integers(1, 5, 256)])
    total = 0
    for call in range(12):
        items = []
        for _ in range(3):
            for s in sts:
                r = rng.random()
                n = 0 if r < 0.1 else 1 if r < 0.2 else int(rng.integers(2, 3001))
                items.append((s, rng.integers(-32768, 32768, n).astype(np.int16)))
        order = rng.permutation(len(items))
        items = [items[k] for k in order]
        got = bank.process(items)
        want = slref.process(procs, items, native=True)
        assert got == want, call
        total += len(got)
    assert total >= 200
    bank.close()


@pytest.mark.gpu
def test_one_measurement_per_call_lag(gpu):
    bank, (s,), procs = _setup(48000, [1])
    x = _tone(440, 0.3, 48000 * 4, 48000)
    got = bank.process([(s, x[:120000])])                                     # 2.5 s: one measurement, not two
    assert [r["frame"] for r in got] == [0] and got == slref.process(procs, [(s, x[:120000])])
    seen = []
    for k in range(10):                                                       # 100 ms frames: the backlog, one per frame
        f = x[120000 + 4800 * k:120000 + 4800 * (k + 1)]
        r = bank.process([(s, f)])
        assert r == slref.process(procs, [(s, f)])
        seen.append(len(r))
    assert seen == [1, 0, 0, 0, 1, 0, 0, 0, 0, 0]                              # 1.5 s carried -> 1.6 s: one; 0.6 s + 4 frames: one
    bank.close()


@pytest.mark.gpu
def test_interval_aggregation(gpu):
    # processor_test.go:153-190 at interval 10: nine seconds give nothing, the tenth one report of 10 measurements
    bank, (s,), procs = _setup(48000, [10])
    rng = np.random.default_rng(3)
    for k in range(11):
        f = (rng.normal(0, 0.1 * (k + 1), 48000) * 32767).clip(-32768, 32767).astype(np.int16)
        got = bank.process([(s, f)])
        assert got == slref.process(procs, [(s, f)])
        assert len(got) == (1 if k == 9 else 0)
        if got:
            bands = got[0]["octave_bands"]
            assert got[0]["duration_seconds"] == 10 and len(bands) == 30
            assert all(b["sample_count"] == 10 and b["min_db"] <= b["mean_db"] <= b["max_db"] for b in bands.values())
    bank.close()


@pytest.mark.gpu
def test_reset_mid_second_drops_the_partial_block(gpu):
    bank, (s,), procs = _setup(32000, [1])
    rng = np.random.default_rng(4)
    a = rng.integers(-20000, 20000, 22400).astype(np.int16)
    b = rng.integers(-20000, 20000, 40000).astype(np.int16)
    assert bank.process([(s, a)]) == []
    bank.reset(s)
    got = bank.process([(s, b)])
    fresh = {s: slref.Processor(32000, 1)}
    assert len(got) == 1 and got == slref.process(fresh, [(s, b)])
    bank.close()


@pytest.mark.gpu
def test_remove_and_add_reuse_a_slot_with_fresh_state(gpu):
    bank, sts, procs = _setup(16000, [1, 2], max_streams=2)
    rng = np.random.default_rng(6)
    x = rng.integers(-30000, 30000, 40000).astype(np.int16)
    bank.process([(sts[0], x[:25000]), (sts[1], x)])
    bank.remove_stream(sts[0])
    with pytest.raises(host.HipError):
        bank.process([(sts[0], x)])
    s2 = bank.add_stream(3)
    assert s2 == sts[0]
    with pytest.raises(host.HipError):
        bank.add_stream(1)                                                    # full
    ref = {s2: slref.Processor(16000, 3)}
    items = [(s2, x), (s2, x), (s2, x[:100])]
    assert bank.process(items) == slref.process(ref, items) != []
    bank.close()


@pytest.mark.gpu
def test_failed_calls_change_nothing(gpu):
    bank, sts, procs = _setup(16000, [1, 1, 2])
    rng = np.random.default_rng(7)
    frames = [(s, rng.integers(-32768, 32768, 20000).astype(np.int16)) for s in sts]
    assert bank.process(frames[:1]) == slref.process(procs, frames[:1])
    with pytest.raises(host.HipError) as e:                                  # two reports, room for one
        bank.process(frames, max_reports=1)
    assert e.value.code == host.E_INVALID
    with pytest.raises(host.HipError):                                       # unknown stream
        bank.process(frames + [(99, frames[0][1])])
    lib = _lib()                                                             # a negative length
    ptrs = (C.c_void_p * 1)(frames[0][1].ctypes.data)
    n_reports = C.c_int(-1)
    reps = (host._SoundLevel * 4)()
    assert lib.bnhip_soundlevel_bank_process_pcm16(bank._h, 1, (C.c_int * 1)(sts[0]), ptrs, (C.c_int * 1)(-5), reps, 4,
                                                   C.byref(n_reports)) == host.E_INVALID and n_reports.value == 0
    for _ in range(2):
        assert bank.process(frames) == slref.process(procs, frames)          # as if the failed calls never happened
    bank.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rate", [16000, 32000, 44100, 48000])
def test_rates(gpu, rate):
    rng = np.random.default_rng(rate)
    bank, sts, procs = _setup(rate, [1, 2, 1, 3, 1])
    for _ in range(3):
        items = [(s, rng.integers(-32768, 32768, int(rng.integers(rate // 4, rate))).astype(np.int16)) for s in sts for _ in range(2)]
        assert bank.process(items) == slref.process(procs, items, native=True)
    assert len(next(iter(bank.process([(sts[0], np.zeros(rate, np.int16))])))["octave_bands"]) == COUNTS[rate]
    bank.close()


@pytest.mark.gpu
def test_silence_is_minus_200_db(gpu):
    bank, (s,), _ = _setup(48000, [2])
    got = bank.process([(s, np.zeros(48000, np.int16)), (s, np.zeros(48000, np.int16))])
    assert len(got) == 1
    for b in got[0]["octave_bands"].values():                                # rms clamped to 1e-10
        assert b["min_db"] == b["max_db"] == b["mean_db"] == -200.0 and b["sample_count"] == 2
    bank.close()


@pytest.mark.gpu
def test_tone_levels(gpu):
    # processor_test.go:113-150: a 1 kHz tone shows in its band at 20 log10(A / sqrt 2), far below it in the 25-100 Hz bands
    amp = 0.5
    bank, (s,), procs = _setup(48000, [1])
    x = _tone(1000, amp, 48000 * 3, 48000)
    reps, ref = [], []
    for k in range(3):                                                        # one 1-second call each
        f = x[48000 * k:48000 * (k + 1)]
        reps += bank.process([(s, f)])
        ref += slref.process(procs, [(s, f)])
    assert reps == ref and len(reps) == 3
    want = 20 * math.log10(amp / math.sqrt(2))
    for r in reps[1:]:                                                        # from the second measurement on
        b = r["octave_bands"]
        assert abs(b["1.0_kHz"]["mean_db"] - want) <= 0.05, b["1.0_kHz"]
        for key in ("25.0_Hz", "31.5_Hz", "40.0_Hz", "50.0_Hz", "63.0_Hz", "80.0_Hz", "100.0_Hz"):
            assert b[key]["mean_db"] < b["1.0_kHz"]["mean_db"] - 20, key
    bank.close()


@pytest.mark.gpu
def test_tone_then_silence_through_subnormals(gpu):
    bank, sts, procs = _setup(48000, [1, 2])
    x = np.concatenate([_tone(15000, 0.9, 30000, 48000), np.zeros(48000 * 2, np.int16)])
    y = np.concatenate([_tone(60, 0.9, 50000, 48000), np.zeros(48000 * 2, np.int16)])
    items = [(sts[0], x[k:k + 9600]) for k in range(0, x.size, 9600)] + [(sts[1], y[:70000]), (sts[1], y[70000:])]
    got = bank.process(items)
    assert got == slref.process(procs, items, native=True) and len(got) >= 3
    st = procs[sts[0]].st
    assert ((st[:, :4] != 0) & (np.abs(st[:, :4]) < 2.2250738585072014e-308)).any()   # the state really went subnormal
    bank.close()
