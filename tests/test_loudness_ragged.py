"""Clip loudness of a ragged burst on the device (bnhip_loudness_ragged_*) against the uniform entries called once per clip and the
float64 restatement of the spec (tests/loudref.py).

Acceptance: at 8 kHz (S = 800) every call here uses the split q = 8, so the ragged entry's records and output samples equal the
uniform entry's, clip by clip, bit for bit; against the restatement the tolerances are those of tests/test_loudness.py
(true_peak bit-equal, every dB field within 1e-9, flags equal, factor within 1e-14 relative, every output sample equal to the
restated gain).  The condition of that file holds here too and is asserted in test_ragged_ref.py: no block energy of these bursts
lies within 1e-6 relative of a gate."""
import ctypes as C
import math

import numpy as np
import pytest

import loudref as R
import raggedcases as K
from birdnet_go_amd import host

from test_loudness import check_measurement, close, fields
from test_parity_gpu import _DevBuf

pytestmark = pytest.mark.gpu
PLANS = {"export": K.EXPORT, "upload": K.UPLOAD}


def run(clips, plan, apply=True):
    return host.loudness_normalize_ragged(clips, K.RATE, plan["T"], plan["C"], plan["max_gain"], plan["gate_fallback"], apply)


def check_against_the_restatement(name, plan, res, out):
    """test_loudness.check_normalized for a list of clips."""
    for i, (s, m, g) in enumerate(zip(K.burst(name), K.measurements(name), res)):
        lift = g.lift_db if g.flags & R.GATE_LIFTED else None
        w = R.normalize(s, K.RATE, plan["T"], plan["C"], plan["max_gain"], plan["gate_fallback"], lift_db=lift, m=m)
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
        assert out[i].dtype == np.int16 and np.array_equal(out[i], R.apply_gain(s, g.factor)), (name, i)
        if g.gain_db == 0.0:
            assert out[i].tobytes() == s.tobytes(), (name, i)


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_equals_the_uniform_entry_clip_by_clip_and_the_restatement(gpu, name, plan):
    clips, p = K.burst(name), PLANS[plan]
    res, out = run(clips, p)
    assert len(res) == len(out) == len(clips)
    for c, s in enumerate(clips):
        (w,), y = host.loudness_normalize(s[None, :], K.RATE, p["T"], p["C"], p["max_gain"], p["gate_fallback"])
        assert fields([res[c]]) == fields([w]), (name, c)
        assert out[c].shape == s.shape and np.array_equal(out[c], y[0]), (name, c)
    check_against_the_restatement(name, p, res, out)
    plan_only, none = run(clips, p, apply=False)
    assert none is None and fields(plan_only) == fields(res)


def test_one_length_equals_the_uniform_entry(gpu):
    clips = K.burst("c")
    for p in PLANS.values():
        res, out = run(clips, p)
        want, y = host.loudness_normalize(np.stack(clips), K.RATE, p["T"], p["C"], p["max_gain"], p["gate_fallback"])
        assert fields(res) == fields(want) and np.array_equal(np.stack(out), y)


def test_the_lift_runs_on_a_strict_subset(gpu):
    res, _ = run(K.burst("d"), K.EXPORT)
    assert any(g.flags & R.GATE_LIFTED for g in res) and not all(g.flags & R.GATE_LIFTED for g in res)
    assert any(g.gain_db != 0.0 for g in res)
    short = run(K.burst("a"), K.EXPORT)[0]
    assert short[0].integrated_lufs == -math.inf and short[0].flags & R.GATE_LIFTED and short[5].flags == 0 and short[5].true_peak == 0.0


def test_device_entry_equals_the_host_entry(gpu):
    clips, p = K.burst("a"), K.EXPORT
    packed, lens = host.ragged_pack(clips)
    B = len(clips)
    want_res, want_out = run(clips, p)
    ws = host.loudness_ragged_workspace_size(lens, K.RATE)
    bufs = d_in, d_out, d_res, d_ws = _DevBuf(packed.nbytes), _DevBuf(packed.nbytes), _DevBuf(B * C.sizeof(host.Loudness)), _DevBuf(ws)
    try:
        d_in.upload(packed)
        with pytest.raises(host.HipError) as e:                              # a workspace one byte too small
            host.loudness_normalize_ragged_device(d_in.ptr, lens, K.RATE, d_res.ptr, d_ws.ptr, ws - 1, d_out.ptr)
        assert e.value.code == host.E_INVALID
        host.loudness_normalize_ragged_device(d_in.ptr, lens, K.RATE, d_res.ptr, d_ws.ptr, ws, d_out.ptr, p["T"], p["C"], p["max_gain"],
                                              p["gate_fallback"])
        out = d_out.download((packed.size,), np.int16)
        raw = d_res.download((B * C.sizeof(host.Loudness),), np.uint8)
    finally:
        for b in bufs:
            b.free()
    res = (host.Loudness * B).from_buffer_copy(raw.tobytes())
    assert fields(res) == fields(want_res) and np.array_equal(out, np.concatenate(want_out))
