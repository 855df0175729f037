"""The fused expand + depthwise layers through the planner, one forced tile shape at a time: the step's own output tensor and its
per-tile squeeze-excite sums against the fp64 oracle.  tests/test_expdw_lab.py pins the kernels on parameter images the lab prepared
itself; this is the only place where the PLANNER's padded images, the orientation strides it hands over and the slab count S that the
sums' consumers index by are checked per shape index rather than per model through logits.

BNHIP_EXPDW_FORCE lives in the create-time tuner, so autotune stays on; each engine forces a different fitting index onto every fused
layer of the model at once (comma list), which bounds the number of engines by the longest candidate list (14) per model."""
import math

import numpy as np
import pytest

from birdnet_go_amd import host, synth_model as sm
from oracle.interp import Interpreter
from oracle.tflite_reader import read_model

from test_expdw_lab import lab, listing, shape_table  # noqa: F401  (fixtures: the lab's --list prints the tile-shape table)

N_CLIPS = 3


def _models():
    from test_parity_gpu import _geo_cfg
    return [("geo1", _geo_cfg(1)), ("geo4", _geo_cfg(4)), ("perch_tiny", sm.tiny_perch_config())]


def _swish_out(m, t):
    """The tensor after a LOGISTIC + MUL pair on t (the graph's swish), or t itself."""
    for lg in m.ops:
        if lg.name == "LOGISTIC" and list(lg.inputs) == [t]:
            for mu in m.ops:
                if mu.name == "MUL" and sorted(mu.inputs) == sorted([t, lg.outputs[0]]):
                    return mu.outputs[0]
    return t


def _dw_output_tensor(m, step_name):
    """TFLite tensor that the fused step `<conv name>+dw` materialises: the depthwise output behind its activation."""
    conv = step_name[:-len("+dw")]
    t = next(o.outputs[0] for o in m.ops if m.tensors[o.outputs[0]].name == conv)
    t = _swish_out(m, t)
    dw = [o for o in m.ops if o.name == "DEPTHWISE_CONV_2D" and o.inputs[0] == t]
    assert len(dw) == 1, step_name
    return _swish_out(m, dw[0].outputs[0])


def _slabs(tiles, idx, Ho, Wo):
    k, s, toh, tow, trh, nw = tiles[idx % len(tiles)]
    if idx >= len(tiles):
        Ho, Wo = Wo, Ho
    return math.ceil(Ho / toh) * math.ceil(Wo / tow)


def _fits(tiles, idx, step):
    """expdw_shape_fits restated: same (k, stride); every tile row's in-image footprint rows within the shape's cap, in the orientation the
    index walks the image; the eight-wave shapes for swish expands whose padded K is 16, 24 or 32 only; the stem in image orientation only."""
    N = len(tiles)
    k, s, toh, tow, trh, nw = tiles[idx % N]
    stem = step["name"] == "stem+dw"
    if (k, s) != (step["k"], step["stride"]) or (stem and idx >= N):
        return False
    kw = (step["C"] + 15) // 16 * 16 if step["C"] % 2 else (step["C"] + 7) // 8 * 8          # expdw_kw: K as the kernel walks it
    if nw == 8 and (stem or step["act"] != 100 or kw not in (16, 24, 32)):
        return False
    H, W = (step["W"], step["H"]) if idx >= N else (step["H"], step["W"])
    Ho = math.ceil(H / s)
    pt = max((Ho - 1) * s + k - H, 0) // 2                       # SAME padding, TensorFlow's rule
    tih = (toh - 1) * s + k
    return all(min(t * toh * s - pt + tih, H) - max(t * toh * s - pt, 0) <= trh for t in range(math.ceil(Ho / toh)))


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1, 2])
def test_forced_tile_shapes_reproduce_the_f64_layer(gpu, monkeypatch, listing, which):
    """Gate, per layer and per forced shape, on err = max|got - ref64| / max|ref64| of the step's output tensor:
        err <= 4 * err_f32 + 2^-16
    where err_f32 is the error of the oracle's own fp32 evaluation of the same tensor (it carries the same upstream accumulation: the
    layer's input is itself a computed fp32 tensor, up to ~16 stages deep, so the kernel-level gate of the lab does not apply here).
    2^-16 covers what the fp32 oracle does not share with the engine: the front end (FFT in fp32 on the device, log / power compression
    on hardware transcendentals) feeds every later layer, and one ulp of fp32 at the spectrogram becomes ~2^-20 ... 2^-17 of a later
    tensor's scale after the swish stack; a structural error of a tile shape (a wrong border pixel, a tap from the padding, a slab
    handed to the wrong consumer) is 1e-3 ... 1 on this scale.  The sums: the same bound times the number of pixels summed, in units
    of the output scale, plus fp32 accumulation.  Measured figures: DESIGN.md."""
    tiles = shape_table(listing)
    N = len(tiles)
    label, cfg = _models()[which]
    blob = sm.build_model(cfg)
    m = read_model(blob)
    x = sm.synth_clips(N_CLIPS, cfg.n_samples, cfg.sample_rate, first=3)
    keep64, keep32 = {}, {}
    Interpreter(m, "f64").invoke(x, keep=keep64)
    Interpreter(m).invoke(x, keep=keep32)

    plan = host.HipClassifier(blob, plan_only=True)
    try:
        layers = [s for s in plan.describe()["steps"] if s["kernel"] == "expand_dw"]
    finally:
        plan.close()
    assert len(layers) >= 4
    # every index is tried on every layer with its (k, stride); the ones the layer accepts must come back from describe() and be checked
    cands = {s["name"]: [i for i in range(2 * N) if tiles[i % N][:2] == (s["k"], s["stride"])] for s in layers}
    fit = {s["name"]: {i for i in range(2 * N) if _fits(tiles, i, s)} for s in layers}
    checked = {s["name"]: set() for s in layers}
    worst = {}
    for rnd in range(max(len(c) for c in cands.values())):
        force = {n: c[rnd] for n, c in cands.items() if rnd < len(c)}
        monkeypatch.setenv("BNHIP_EXPDW_FORCE", ",".join(f"{n}={i}" for n, i in force.items()))
        clf = host.HipClassifier(blob, max_batch=4, lanes=1, debug_no_reuse=True)
        try:
            steps = {s["name"]: s for s in clf.describe()["steps"] if s["kernel"] == "expand_dw"}
            clf.predict_batch(x.reshape(-1), N_CLIPS)
            for name, idx in force.items():
                s = steps[name]
                if s["shape"] != idx:                          # refused: only what the layer does not fit may be (the tuner then keeps its own)
                    assert idx not in fit[name], (label, name, idx, s["shape"])
                    continue
                Ho, Wo, C = math.ceil(s["H"] / s["stride"]), math.ceil(s["W"] / s["stride"]), s["Co"]
                ti = _dw_output_tensor(m, name)
                ref = np.asarray(keep64[ti], np.float64).reshape(N_CLIPS, Ho * Wo, C)
                r32 = np.asarray(keep32[ti], np.float64).reshape(ref.shape)
                got = clf.debug_fetch(-2 - s["out_v"], N_CLIPS, Ho * Wo * C).astype(np.float64).reshape(ref.shape)
                scale = float(np.abs(ref).max())
                err, e32 = float(np.abs(got - ref).max()) / scale, float(np.abs(r32 - ref).max()) / scale
                gate = 4 * e32 + 2.0 ** -16
                assert s["fused_sum"] == 1 and s["out2_v"] >= 0
                S = _slabs(tiles, idx, Ho, Wo)
                raw = clf.debug_fetch(-2 - s["out2_v"], N_CLIPS, 64 * C * 64).reshape(-1)
                sums = raw[:N_CLIPS * S * C].astype(np.float64).reshape(N_CLIPS, S, C).sum(axis=1)
                rsum = ref.sum(axis=1)
                serr = float(np.abs(sums - rsum).max()) / scale
                sgate = Ho * Wo * (gate + 2.0 ** -24)
                print(f"{label} {name} shape {idx}: y err {err:.3e} (fp32 oracle {e32:.3e}, gate {gate:.3e}); sums err {serr:.3e} of the y scale (gate {sgate:.3e}), S = {S}")
                w = worst.setdefault(name, [0.0, 0.0, 0.0])
                w[0], w[1], w[2] = max(w[0], err), max(w[1], e32), max(w[2], serr / (Ho * Wo))
                assert np.isfinite(got).all() and err <= gate, (label, name, idx, err, e32)
                assert np.isfinite(sums).all() and serr <= sgate, (label, name, idx, serr, sgate)
                checked[name].add(idx)
        finally:
            clf.close()
    for name, w in worst.items():
        print(f"{label} {name}: {len(checked[name])} shapes {sorted(checked[name])}, worst y err {w[0]:.3e} (fp32 oracle {w[1]:.3e}), worst sums err per pixel {w[2]:.3e}")
    # exactly the indices each layer fits were forced, reported back and compared - no more, no fewer
    for s in layers:
        assert checked[s["name"]] == fit[s["name"]] and len(fit[s["name"]]) >= (3 if s["name"] == "stem+dw" else 4), \
            (label, s["name"], sorted(checked[s["name"]]), sorted(fit[s["name"]]))
