"""Clip loudness on the device (bnhip_loudness_*) against the float64 restatement of the spec (tests/loudref.py).

Acceptance, per clip: true_peak bit-equal (same order, nothing fused: a mismatch is a wrong tap or order); every dB field within
1e-9; sub_energy within 1e-9 relative - of the clip's largest sub-block energy, the project's form of this bound
(test_us_device.py) - which leaves >= 40 x over the scan's measured rounding (2.4e-11 LU, 1.3e-11 relative: DESIGN.md section 9); flags
equal; factor
within 1e-14 relative of pow(10, gain_db / 20) and exactly 1 at 0 dB; every output byte equal to pcmgain restated with the reported
factor.  For a lifted clip the restatement builds the lifted clip from the reported lift_db.
A condition, not a tolerance: every block energy of every case lies at least 1e-6 relative from both gates in the restatement
(asserted first), so no gate decision can flip and no case is excused."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import loudref as R
from birdnet_go_amd import host, loudness

from test_parity_gpu import _DevBuf

pytestmark = pytest.mark.gpu
INF = math.inf
EXPORT = dict(T=-23.0, C=-1.0, max_gain=60.0, gate_fallback=True)        # actions_database.go:1392-1438
UPLOAD = dict(T=-23.0, C=-1.0, max_gain=30.0, gate_fallback=False)       # encode_native.go:25-66


def tone(rate, n, hz, amp, phase=0.0):
    return np.round(amp * 32767.0 * np.sin(2.0 * np.pi * hz * np.arange(n) / rate + phase)).astype(np.int16)


def noise(rng, n, amp):
    return np.clip(np.round(rng.standard_normal(n) * amp * 32768.0), -32768, 32767).astype(np.int16)


def mixed(rate, n, i, seed):
    """Clip i of a batch: tone / noise with a quiet third / modulated noise in turn, another amplitude and pitch each time."""
    rng = np.random.default_rng(1000 * seed + i)
    amp = (0.9, 0.05, 0.3, 0.01, 0.6)[i % 5]
    kind = i % 3
    if kind == 0:
        return tone(rate, n, 180.0 + 97.0 * i, amp, 0.3 * i)
    if kind == 1:
        x = noise(rng, n, amp / 3.0)
        a, b = n // 3, 2 * n // 3
        x[a:b] = noise(rng, b - a, amp / 3000.0)
        return x
    x = noise(rng, n, amp / 3.0).astype(np.float64) * (0.55 + 0.45 * np.sin(2.0 * np.pi * 2.7 * np.arange(n) / rate + i))
    return np.round(x).astype(np.int16)


def batch(rate, n, count, seed):
    return np.stack([mixed(rate, n, i, seed) for i in range(count)])


def sub_gate(n, seed, lo=-3, hi=3):
    return np.random.default_rng(seed).integers(lo, hi + 1, n).astype(np.int16)


def sparse_clicks(n, every):
    x = np.zeros(n, np.int16)
    x[every // 2::every] = 1
    return x


def square(n, half_period=8):
    return np.where((np.arange(n) // half_period) % 2 == 0, 32767, -32768).astype(np.int16)


def tail_peak(rate, n):
    """A quiet tone whose loudest sample and an inter-sample peak (fs / 4 at 45 degrees: + + - -) lie in the trailing partial sub-block."""
    S = R.sub_block(rate)
    x = tone(rate, n, 440.0, 0.05)
    x[4 * S + 40:4 * S + 48] = np.array([1, 1, -1, -1, 1, 1, -1, -1], np.int16) * 30000
    x[4 * S + 100] = 32767
    return x


def last_sample_peak(rate, n):
    x = tone(rate, n, 300.0, 0.02)
    x[-3:] = [-20000, 26000, 30000]
    return x


def contents(rate, n):
    """The special contents as one batch: zeros, sub-gate (lifted and refined), sub-gate that stays under the gate after the lift,
    full-scale square wave, all -32768."""
    return np.stack([np.zeros(n, np.int16), sub_gate(n, 7), sparse_clicks(n, 4 * R.sub_block(rate)), square(n), np.full(n, -32768, np.int16),
                     sub_gate(n, 8, -1, 1)])


def sixty_five(rate, n):
    x = batch(rate, n, 65, 5)
    x[[9, 33, 64]] = np.stack([np.zeros(n, np.int16), sub_gate(n, 9), sparse_clicks(n, 4 * R.sub_block(rate))])
    return x


S8 = 800
CASES = {
    # name: (rate, clips builder, plan)
    "n1": (8000, lambda: np.array([[-32768], [17], [0]], np.int16), EXPORT),
    "n31": (8000, lambda: batch(8000, 31, 3, 1), EXPORT),
    "n32": (8000, lambda: batch(8000, 32, 3, 2), EXPORT),
    "n33": (8000, lambda: batch(8000, 33, 3, 3), EXPORT),
    "no_block": (8000, lambda: batch(8000, 4 * S8 - 1, 3, 4), EXPORT),                  # finite peak, -inf loudness
    "one_block": (8000, lambda: batch(8000, 4 * S8, 3, 5), EXPORT),
    "ignored_tail": (8000, lambda: np.stack([tail_peak(8000, 4 * S8 + S8 // 2)]), UPLOAD),
    "drain": (8000, lambda: np.stack([last_sample_peak(8000, 5 * S8 + 11), last_sample_peak(8000, 5 * S8 + 11)[::-1].copy()]), UPLOAD),
    "two_tiles_one_clip": (8000, lambda: batch(8000, 70 * S8 + 123, 1, 6), UPLOAD),     # 70 segments: 2 blocks, the scan crosses them
    "sixty_five": (8000, lambda: sixty_five(8000, 5 * S8 + 37), EXPORT),                # 325 segments: 6 blocks, the last one partial
    "contents": (8000, lambda: contents(8000, 6 * S8 + 5), EXPORT),
    "contents_unbounded": (8000, lambda: contents(8000, 6 * S8 + 5), dict(T=-23.0, C=-1.0, max_gain=INF, gate_fallback=True)),
    "contents_upload": (8000, lambda: contents(8000, 6 * S8 + 5), UPLOAD),              # no fallback: 0 dB, copies
    "square_peak_limited": (8000, lambda: np.stack([square(5 * S8), square(5 * S8, 3)]), dict(T=-0.5, C=-1.0, max_gain=30.0, gate_fallback=False)),
    "clamp30": (8000, lambda: np.stack([tone(8000, 5 * S8, 500.0, 0.001)]), UPLOAD),                                  # wanted ~ +40
    "clamp30_down": (8000, lambda: np.stack([tone(8000, 5 * S8, 500.0, 0.9)]), dict(T=-60.0, C=-1.0, max_gain=30.0, gate_fallback=False)),
    "r11025": (11025, lambda: batch(11025, 7 * 1103 + 551, 3, 7), EXPORT),              # S = 1103
    "r44100": (44100, lambda: batch(44100, 6 * 4410 + 1000, 3, 8), EXPORT),
    "r48000": (48000, lambda: batch(48000, 5 * 4800 + 4799, 3, 9), UPLOAD),
    "r256000": (256000, lambda: batch(256000, 5 * 25600 + 77, 1, 10), EXPORT),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (rate, clips, plan, the restatement's measurement of every clip): built once, shared by every test, never changed."""
    rate, build, plan = CASES[name]
    clips = build()
    clips.setflags(write=False)
    return rate, clips, plan, tuple(R.measure(s, rate) for s in clips)


def close(a, b, tol=1e-9):
    return a == b or abs(a - b) <= tol


def check_measurement(name, i, got, m, sub=None):
    assert m["margin"] >= 1e-6, (name, i, "a block energy sits on a gate", m["margin"])
    assert got.true_peak == m["P"], (name, i, got.true_peak, m["P"])
    assert close(got.integrated_lufs, m["L"]) and close(got.true_peak_dbtp, m["dbtp"]), (name, i, got.integrated_lufs, m["L"], got.true_peak_dbtp, m["dbtp"])
    if sub is not None:
        assert sub.shape == m["E"].shape
        if sub.size:
            assert np.abs(sub - m["E"]).max() <= 1e-9 * np.abs(m["E"]).max(), (name, i)


def check_normalized(name, res, out, check_bytes=True):
    rate, clips, plan, meas = case(name)
    assert len(res) == len(clips)
    for i, (s, m, g) in enumerate(zip(clips, meas, res)):
        lift = g.lift_db if g.flags & R.GATE_LIFTED else None
        w = R.normalize(s, rate, plan["T"], plan["C"], plan["max_gain"], plan["gate_fallback"], lift_db=lift, m=m)
        assert w["margin"] >= 1e-6, (name, i, "a block energy sits on a gate", w["margin"])
        check_measurement(name, i, g, m)
        assert g.flags == w["flags"], (name, i, g.flags, w["flags"])
        if lift is not None:
            assert close(g.lift_db, w["own_lift_db"]), (name, i)
        for f in ("target_gain_db", "lift_db", "planned_gain_db", "gain_db", "output_lufs"):
            assert close(getattr(g, f), w[f]), (name, i, f, getattr(g, f), w[f])
        if g.gain_db == 0.0:
            assert g.factor == 1.0, (name, i)
        else:
            assert abs(g.factor - math.pow(10.0, g.gain_db / 20.0)) <= 1e-14 * math.pow(10.0, g.gain_db / 20.0), (name, i, g.factor)
        if check_bytes:
            assert out[i].dtype == np.int16 and np.array_equal(out[i], R.apply_gain(s, g.factor)), (name, i)
            if g.gain_db == 0.0:
                assert out[i].tobytes() == s.tobytes(), (name, i)


@pytest.mark.parametrize("name", list(CASES))
def test_measure(gpu, name):
    rate, clips, _, meas = case(name)
    res, sub = host.loudness_measure(clips, rate, sub_energy=True)
    assert sub.shape == (len(clips), clips.shape[1] // R.sub_block(rate))
    for i, (g, m) in enumerate(zip(res, meas)):
        check_measurement(name, i, g, m, sub[i])
        assert (g.gain_db, g.factor, g.flags) == (0.0, 1.0, 0) and close(g.output_lufs, m["L"])


@pytest.mark.parametrize("name", list(CASES))
def test_normalize(gpu, name):
    rate, clips, plan, _ = case(name)
    res, out = host.loudness_normalize(clips, rate, plan["T"], plan["C"], plan["max_gain"], plan["gate_fallback"])
    check_normalized(name, res, out)


def fields(res):
    return [tuple(getattr(g, f) for f, _ in host.Loudness._fields_) for g in res]


def test_the_cases_reach_every_branch(gpu):
    """What the table above is there for, checked on the device's own answers."""
    def run(name):
        rate, clips, plan, _ = case(name)
        return host.loudness_normalize(clips, rate, plan["T"], plan["C"], plan["max_gain"], plan["gate_fallback"])[0]
    zeros, lifted, stays, sq, dc, ones = run("contents")
    assert zeros.flags == 0 and zeros.true_peak == 0.0 and zeros.gain_db == 0.0 and zeros.output_lufs == -INF
    assert lifted.flags & R.GATE_LIFTED and lifted.integrated_lufs == -INF and lifted.planned_gain_db > lifted.lift_db
    assert stays.flags == R.GATE_LIFTED and stays.planned_gain_db == stays.lift_db == 47.0 and stays.output_lufs == -INF
    assert sq.true_peak_dbtp > 0.0 and dc.true_peak >= 1.0
    assert ones.flags == R.GATE_LIFTED | R.CLAMPED and ones.gain_db == 60.0                 # clamp at 60
    unb = run("contents_unbounded")
    assert unb[5].flags == R.GATE_LIFTED and unb[5].gain_db == unb[5].planned_gain_db > 60.0
    assert all(g.gain_db == 0.0 and g.flags == 0 for g in (run("contents_upload")[i] for i in (0, 1, 2, 5)))      # gain_db == 0
    assert all(g.flags & R.PEAK_LIMITED and g.true_peak_dbtp > 0.0 for g in run("square_peak_limited"))
    quiet, loud = run("clamp30")[0], run("clamp30_down")[0]
    assert (quiet.gain_db, loud.gain_db, quiet.flags, loud.flags) == (30.0, -30.0, R.CLAMPED, R.CLAMPED)   # clamp at 30
    tail = run("ignored_tail")[0]
    assert tail.true_peak > 1.0 and tail.flags & R.PEAK_LIMITED
    assert all(g.integrated_lufs == -INF and g.true_peak > 0.0 for g in run("no_block"))
    assert all(g.integrated_lufs > -70.0 for g in run("one_block"))


@pytest.mark.parametrize("name", ["contents", "sixty_five", "r11025"])
def test_plan_only_equals_the_applied_call(gpu, name):
    rate, clips, plan, _ = case(name)
    args = (clips, rate, plan["T"], plan["C"], plan["max_gain"], plan["gate_fallback"])
    res, out = host.loudness_normalize(*args, apply=False)
    assert out is None and fields(res) == fields(host.loudness_normalize(*args)[0])
    check_normalized(name, res, None, check_bytes=False)


@pytest.mark.parametrize("name", ["contents", "sixty_five", "n33", "r44100"])
def test_device_entry_equals_the_host_entry(gpu, name):
    rate, clips, plan, _ = case(name)
    B, n = clips.shape
    want_res, want_out = host.loudness_normalize(clips, rate, plan["T"], plan["C"], plan["max_gain"], plan["gate_fallback"])
    ws = host.loudness_workspace_size(B, n, rate)
    bufs = d_in, d_out, d_res, d_ws = _DevBuf(clips.nbytes), _DevBuf(clips.nbytes), _DevBuf(B * C.sizeof(host.Loudness)), _DevBuf(ws)
    try:
        d_in.upload(np.ascontiguousarray(clips))
        host.loudness_normalize_device(d_in.ptr, B, n, rate, d_res.ptr, d_ws.ptr, ws, d_out.ptr, plan["T"], plan["C"], plan["max_gain"],
                                       plan["gate_fallback"])
        out = d_out.download((B, n), np.int16)
        raw = d_res.download((B * C.sizeof(host.Loudness),), np.uint8)
    finally:
        for b in bufs:
            b.free()
    res = (host.Loudness * B).from_buffer_copy(raw.tobytes())
    assert fields(res) == fields(want_res) and np.array_equal(out, want_out)


def test_normalize_clips_groups_a_burst_by_length(gpu):
    rate, a, _, _ = case("one_block")
    _, b, _, _ = case("contents")
    burst = [a[0], b[1], a[1], b[3], a[2]]
    res, out = loudness.normalize_clips(burst, rate, max_gain_db=loudness.EXPORT_MAX_GAIN_DB, gate_fallback=True)
    ra, oa = host.loudness_normalize(a, rate, -23.0, -1.0, 60.0, True)
    rb, ob = host.loudness_normalize(b[[1, 3]], rate, -23.0, -1.0, 60.0, True)
    assert fields(res) == fields([ra[0], rb[0], ra[1], rb[1], ra[2]])
    for got, want in zip(out, [oa[0], ob[0], oa[1], ob[1], oa[2]]):
        assert np.array_equal(got, want)
    res, out = loudness.normalize_clips(burst, rate, apply=False)
    assert out is None and len(res) == 5 and not any(g.flags & R.GATE_LIFTED for g in res)


def test_coefficient_table_evicted_and_rebuilt(gpu):
    """The table cache holds 32 entries and the oldest leaves: 40 rates evict and rebuild the first one."""
    rng = np.random.default_rng(40)
    clip = noise(rng, 3300, 0.1)[None, :]                         # about four sub-blocks at 8 kHz
    first = bytes(host.loudness_measure(clip, 8000)[0])
    for i in range(1, 40):
        last = host.loudness_measure(clip, 8000 + i, sub_energy=True)
    assert bytes(host.loudness_measure(clip, 8000)[0]) == first
    (g,), sub = last
    check_measurement("evict", 0, g, R.measure(clip[0], 8039), sub[0])
    assert (g.gain_db, g.factor, g.flags) == (0.0, 1.0, 0)
