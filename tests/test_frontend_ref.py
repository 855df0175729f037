"""The front-end reference (tests/feref.py) and its gate, tested on the CPU for every case of tests/fecases.py before any device is
held to them: (a) the reference agrees with the existing oracle, (b) the gate is not vacuous, (c) the gate has teeth."""
import numpy as np
import pytest

import fecases
import feref
from oracle.interp import Interpreter
from oracle.tflite_reader import read_model

MUTATIONS = ["last_frame_early", "window_tap", "band_shift", "bin_plus_one", "swap_channels", "repeat_frame", "mel_order"]

_cache = {}


def _setup(case):
    """(model, clips, live clips, reference) of a case, computed once and shared (never modified) by the three tests."""
    if case.name not in _cache:
        _cache.clear()                                   # tests run case by case: keep one case's arrays at a time
        m = read_model(fecases.model(case))
        x, live = fecases.clips(case, fecases.N_CPU)
        _cache[case.name] = (m, x, live, feref.front_end(case.cfg, m, x, case.eps_t))
    return _cache[case.name]


def _spec_tensor(m):
    return next(o for o in m.ops if o.name == "CONV_2D").inputs[0]


@pytest.mark.parametrize("case", fecases.CASES, ids=lambda c: c.name)
def test_reference_agrees_with_the_oracle(case):
    """The fp32 oracle's spectrogram (TFLite semantics: fp32 mel product, fp32 log / pow) lies inside the interval at every pixel.
    The fp64 oracle differs from the reference by what it does NOT round: it normalises and windows in fp64 where the graph (and
    the reference) round each of the five normalising operations and the window product to fp32 - per sample at most
    2^-24 (7 w[n] + |frame[n]|) when the clip is normalised (|x - min| / d <= 1: SUB, DIV, SUB each within 2^-24 of a value <= 1,
    doubled by the MUL 2, the divisor's own two roundings on top) and 2^-24 |frame[n]| for the window product alone - and it does
    not narrow the bins (2^-24 |x^_k|).  Its image must lie inside the interval of that bound."""
    cfg = case.cfg
    m, x, live, ref = _setup(case)
    st = _spec_tensor(m)
    keep = {}
    Interpreter(m).invoke(x, keep=keep)
    img32 = np.asarray(keep[st], np.float64)
    assert img32.shape == ref.mid.shape
    worst, n_out, _ = feref.check_image(img32, ref)
    assert n_out == 0, (case.name, worst, n_out)
    keep = {}
    Interpreter(m, "f64").invoke(x, keep=keep)
    img64 = np.asarray(keep[st], np.float64)
    los, his = [], []
    for ch in ref.chans:
        w = np.abs(ch.mel.astype(np.float64))
        A = np.abs(ch.frames.astype(np.float64)).sum(axis=-1)[..., None]
        per_frame = 2.0 ** -24 * (A + (7.0 * ch.win_sum if cfg.normalize else 0.0))
        tw = 2.0 ** -24 * (np.abs(ch.bins.astype(np.float64)) @ w.T) + per_frame * w.sum(axis=1)[None, None, :]
        lo, hi = feref.pixel_interval(cfg, ch.v, tw)
        los.append(lo); his.append(hi)
    ref64 = feref.FrontRef(None, None, ref.chans, ref.mid, feref.layout(cfg, los), feref.layout(cfg, his))
    worst, n_out, _ = feref.check_image(img64, ref64)
    assert n_out == 0, (case.name, worst, n_out)


@pytest.mark.parametrize("case", fecases.CASES, ids=lambda c: c.name)
def test_gate_is_not_vacuous(case):
    """At most 1 % of the pixels may have an interval wider than 1e-3 of the image's maximum."""
    m, x, live, ref = _setup(case)
    width = ref.hi - ref.lo
    top = float(np.abs(ref.mid).max())
    share = float((width > 1e-3 * top).mean())
    print(f"{case.name}: median width / max {np.median(width) / top:.2e}, widest {width.max() / top:.2e}, share above 1e-3: {share:.4f}")
    assert np.isfinite(width).all() and (width >= 0).all() and top > 0
    assert share <= 0.01, (case.name, share)


@pytest.mark.parametrize("case", fecases.CASES, ids=lambda c: c.name)
def test_gate_has_teeth(case):
    """A reference recomputed with one structural error must fall outside the intervals on every live clip (the silent, constant,
    half-silent, impulse and pure-tone clips are exempt by construction: a shifted reference of silence is silence).  Swapping the
    channels needs two; reversing the mel order is the error whichever order the layout has.  One pixel moved by 4 tau: tau taken
    as the pixel's own tolerance in the image, half its interval's width (in the mel sum's units the hardware-ulp widening of the
    interval can exceed 3 tau of a quiet band, and a move that small is then allowed by derivation); the loudest pixel of a live
    clip, moved either way - that pixel and no other must be outside, by 1.5 widths.  A NaN is outside."""
    cfg = case.cfg
    m, x, live, ref = _setup(case)
    assert feref.check_image(ref.mid, ref)[1] == 0
    for mut in MUTATIONS:
        if mut == "swap_channels" and len(cfg.specs) < 2:
            continue
        bad = feref.front_end(cfg, m, x, case.eps_t, mutate=mut)
        _, _, excess = feref.check_image(bad.mid, ref)
        per_clip = (excess.reshape(excess.shape[0], -1) > 0).sum(axis=1)
        assert all(per_clip[i] > 0 for i in live), (case.name, mut, per_clip.tolist())
    # one pixel moved by four times its tolerance
    mag = np.abs(ref.mid).copy()
    mag[[i for i in range(x.shape[0]) if i not in live]] = -1.0
    at = np.unravel_index(int(mag.argmax()), mag.shape)
    half = 0.5 * (ref.hi[at] - ref.lo[at])
    assert half > 0
    for sign in (1.0, -1.0):
        moved = ref.mid.copy()
        moved[at] = 0.5 * (ref.hi[at] + ref.lo[at]) + sign * 4.0 * half
        worst, n_out, excess = feref.check_image(moved, ref)
        assert n_out == 1 and excess[at] > 0 and 1.4 < worst < 1.6, (case.name, n_out, worst)
    nan = ref.mid.copy()
    nan[at] = np.nan
    assert feref.check_image(nan, ref)[1] == 1
