"""Every kernel form of the mel front end held to the fp64 reference (tests/feref.py) at the tensors the kernels write: the
(min, range + eps) pair and the normalised clip bit for bit, the STFT bins tensor within the derived tolerance per bin with its
padding columns exactly zero, and every pixel of the spectrogram image inside its derived interval.  One engine per case of
tests/fecases.py (debug_no_reuse: every step's output keeps its own memory; autotune off; one lane), the plan checked for the kernel
form the case is in the table for.  Measured worst ratios: DESIGN.md."""
import math

import numpy as np
import pytest

import fecases
import feref
from birdnet_go_amd import host
from oracle.tflite_reader import read_model

pytestmark = pytest.mark.gpu

FRONT_KERNELS = ("clip_minmax", "stft", "frontend")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _fetch(clf, step, n, elems):
    got = clf.debug_fetch(-2 - step["out_v"], n, elems)
    assert got.shape == (n, elems), (step["name"], got.shape, elems)
    return got


def _check_plan(case, d, n, consts):
    """The plan took the form the case is in the table for: the front-end steps by name and kernel class, the geometry the planner
    read from the graph, and - restated from the launch code - the frames per wave, the fused epilogue's limits and the mel tile count."""
    cfg = case.cfg
    steps = d["steps"]
    k = len(case.steps)
    assert [s["name"] for s in steps[:k]] == case.steps, [s["name"] for s in steps[:k + 1]]
    assert steps[k]["kernel"] not in FRONT_KERNELS and not steps[k]["name"].startswith("mel"), steps[k]
    for s in steps[:k]:
        want = ("clip_minmax" if s["name"] == "clip_minmax" else "stft" if s["name"].startswith("stft") else
                "pw_gemm" if s["name"].startswith("mel") and s["name"][3:].isdigit() else "frontend")
        assert s["kernel"] == want, s
    assert d["precision"] == case.eng.get("precision", "f32") and d["lanes"] == 1
    n_pad = cfg.n_samples + sum(cfg.pad)
    for sp, fs, (win, mel) in zip(cfg.specs, d["specs"], consts):
        N = sp.fft_length or sp.frame_length
        F = 1 + (n_pad - sp.frame_length) // sp.frame_step
        assert (fs["frame_length"], fs["fft_length"], fs["hop"], fs["frames"], fs["n_mels"]) == (sp.frame_length, N, sp.frame_step, F, cfg.n_mels), fs
    fft_path = any(nm.startswith("stft") for nm in case.steps)
    F = d["specs"][0]["frames"]
    if fft_path:
        assert all((sp.fft_length or sp.frame_length) in (512, 1024, 2048) for sp in cfg.specs)
        fpw = min(max(math.ceil(F * n / 2048), 1), 16)                     # launch_stft_bins
        assert fpw == case.fpw, (fpw, case.fpw)
        if fpw > 1:
            waves = 8                                                       # 512-point blocks: the last block's waves run past F
            assert math.ceil(F / (waves * fpw)) * waves * fpw > F
        for c, (win, mel) in enumerate(consts):
            need = feref.needed_bins(mel)
            nbp = (need.size + 3) // 4 * 4
            fits = nbp <= 512 and feref.mel_quads(mel, need) <= 256         # stft_mel_table
            if "BNHIP_FUSE_MEL" in case.env:
                assert (f"stft{c}+mel" in case.steps) == fits, (case.name, nbp, feref.mel_quads(mel, need))
        if case.nb:
            assert tuple(feref.needed_bins(mel).size for _, mel in consts) == case.nb
        if case.eng.get("precision") == "bf16":
            assert cfg.compress == "log" and "BNHIP_FUSE_MEL" not in case.env      # what selects k_stft_bins<.., float> (Engine::run)
    else:
        assert cfg.complex_mode == "real" and cfg.normalize and cfg.compress == "pow" and not cfg.time_major and cfg.pad == (0, 0)
        assert case.eng.get("frontend_fft") == 0 or all((sp.fft_length or sp.frame_length) in (256, 384) for sp in cfg.specs)
        assert f"k_frontend<{(cfg.n_mels + 15) // 16}," in case.reaches or "k_frontend scalar" in case.reaches, case.reaches


def _run(case, monkeypatch, extra_env=None, only_norm=False):
    """One engine, one call (two with case.twice); every assertion of the module docstring.  Returns the fetched tensors."""
    cfg = case.cfg
    n = case.n_clips
    blob = fecases.model(case)
    m = read_model(blob)
    consts = feref.model_consts(m, len(cfg.specs))
    x, _ = fecases.clips(case, n)
    half_img = False
    for k, v in {**case.env, **(extra_env or {})}.items():
        monkeypatch.setenv(k, v)
    clf = host.HipClassifier(blob, max_batch=n, lanes=1, debug_no_reuse=True, autotune=False, **case.eng)
    out = {}
    try:
        d = clf.describe()
        _check_plan(case, d, n, consts)
        steps = {s["name"]: s for s in d["steps"][:len(case.steps)]}
        half_img = bool(steps[case.steps[-1]]["out_bf16"])
        ref = feref.front_end(cfg, m, x, case.eps_t, half_out=half_img)
        for rep in range(2 if case.twice else 1):
            logits = clf.predict_batch(x.reshape(-1), n)
            assert np.isfinite(logits).all()
            if cfg.normalize:
                mm = _fetch(clf, steps["clip_minmax"], n, 2)
                assert np.array_equal(mm[:, 0], ref.mm[:, 0]), (case.name, rep, "min")                   # (the sign of a zero minimum is free)
                assert np.array_equal(_bits(mm[:, 1]), _bits(ref.mm[:, 1])), (case.name, rep, "range + eps")
                out["mm"] = mm
                if "normalize" in steps:
                    xn = _fetch(clf, steps["normalize"], n, cfg.n_samples)
                    bad = np.flatnonzero(_bits(xn) != _bits(ref.xn))
                    assert bad.size == 0, (case.name, rep, "xn", bad.size, bad[:4])
                    out["xn"] = xn
        if cfg.normalize and "normalize" in steps:
            # which form ran, from the per-step profile (as tests/test_norm_resident.py reads it): the resident launch leaves the
            # normalize step without a launch of its own - above 16 clips of a whole number of quads, when switched on
            clf.profile_enable(True)
            try:
                clf.predict_batch(x.reshape(-1), n)
                launched = {r["name"] for r in clf.profile_read(per_step=True)[1]}
            finally:
                clf.profile_enable(False)
            resident = (extra_env or {}).get("BNHIP_NORM_RESIDENT") != "0" and n > 16 and cfg.n_samples % 4 == 0
            assert "clip_minmax" in launched and ("normalize" in launched) != resident, (case.name, sorted(launched)[:6], resident)
            out["resident"] = resident
        if only_norm:
            return out
        worst_bin, fails = 0.0, []                                          # (every figure is printed before the case is judged)
        for c, ch in enumerate(ref.chans):
            s = steps.get(f"stft{c}")
            if s is None:
                continue
            assert s["out_bf16"] == 0
            nb = ch.needed.size
            nbp = (nb + 3) // 4 * 4
            F = ch.bins.shape[1]
            bins = _fetch(clf, s, n, F * nbp)
            ratio, pad_nonzero = feref.check_bins(bins, ch, nbp)
            worst_bin = max(worst_bin, ratio)
            if pad_nonzero:
                fails.append((f"bins{c}: non-zero padding columns", pad_nonzero))
            if not ratio <= 1.0:
                fails.append((f"bins{c}: worst error / tolerance", ratio))
            out[f"bins{c}"] = bins
        st = next(o for o in m.ops if o.name == "CONV_2D").inputs[0]
        elems = int(np.prod(ref.mid.shape[1:]))
        raw = clf.debug_fetch(st, n, elems)
        if half_img:                                                       # bf16 storage: the first half of the bytes, widened
            img = (raw.reshape(-1).view(np.uint16)[:n * elems].astype(np.uint32) << 16).view(np.float32)
        else:
            img = raw
        img = img.reshape(ref.mid.shape)
        out["img"] = img
        worst, n_out, excess = feref.check_image(img, ref)
        width = ref.hi - ref.lo
        with np.errstate(divide="ignore", invalid="ignore"):
            signed = np.where(width > 0, np.maximum(ref.lo - img, img - ref.hi) / width, -np.inf)       # (-0.5: the middle)
        print(f"FE-RATIO {case.name}{'' if not extra_env else ' ' + str(extra_env)}: bins err / tol {worst_bin:.3f}; pixels outside {n_out} of {img.size}, "
              f"worst excess / width {worst:.3f}, nearest an end, in widths (negative: inside) {float(np.nanmax(signed)):+.3f}")
        if not np.isfinite(img).all():
            fails.append(("image: non-finite pixels", int((~np.isfinite(img)).sum())))
        if n_out:
            at = np.unravel_index(int(excess.argmax()), excess.shape)
            fails.append(("image: pixels outside", n_out, "by clip", (excess.reshape(n, -1) > 0).sum(axis=1).tolist(), "worst at [clip, h, w, c]",
                          tuple(int(i) for i in at), float(img[at]), float(ref.lo[at]), float(ref.hi[at])))
        assert not fails, (case.name, fails)
        return out
    finally:
        clf.close()


@pytest.mark.parametrize("case", fecases.CASES, ids=lambda c: c.name)
def test_front_end_tensors_vs_f64(gpu, monkeypatch, case):
    if case.name.startswith("prune_"):
        # both forms inside the gate, and the pruned closing stage bit-identical to the full one
        a = _run(case, monkeypatch, {"BNHIP_STFT_PRUNE": "1"})
        b = _run(case, monkeypatch, {"BNHIP_STFT_PRUNE": "0"})
        assert np.array_equal(_bits(a["bins0"]), _bits(b["bins0"])) and np.array_equal(_bits(a["img"]), _bits(b["img"]))
        return
    on = _run(case, monkeypatch, {"BNHIP_NORM_RESIDENT": "1"})
    if "normalize" in case.steps:
        # the pair of launches against the one resident launch (taken above 16 clips of a whole number of quads): same bits, both the reference's
        off = _run(case, monkeypatch, {"BNHIP_NORM_RESIDENT": "0"}, only_norm=True)
        assert np.array_equal(_bits(on["xn"]), _bits(off["xn"])) and np.array_equal(_bits(on["mm"]), _bits(off["mm"]))
        assert not off["resident"] and on["resident"] == (case.name == "minmax_vec_resident")
