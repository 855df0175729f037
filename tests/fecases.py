"""Case table of the front-end spectrogram tests (tests/test_frontend_ref.py on the CPU, tests/test_frontend_spectrogram.py on the
GPU): the smallest model per kernel form of the mel front end, each with the form it is meant to reach.  The backbone behind the
spectrogram is as small as the builder makes one - nothing behind the first convolution's input is compared here.

What the table cannot hold, and why:
  * 513 needed bins under a 1024-point transform: the builder's bank (tf.signal.linear_to_mel_weight_matrix) gives the DC bin no
    weight, so 512 (bins 1..512, upper edge above Nyquist) is the most a 1024-point bank reads; 511 and 512 are both in the table.
    The loop beyond 512 bins therefore starts with the 2048-point transform (nbp > 512 needs nb >= 509 AND a fifth quad row).
  * k_stft_bins<.., MEL = true, R = float>: not instantiated (the fp32 transform serves the non-fused form only).
  * k_frontend<NT, WN, 64, 16>: taken only when the 64-frame shape is forced onto a layer whose padded K is a multiple of 16 but
    not of 32; the planner pads K to 32 whenever the 32-frame shape does not fit, so without BNHIP_FE_SHAPE it is unreachable.
  * k_frontend<NT, WN, 64, 32> for NT = 1, 3..6: reachable only with hops of several hundred samples under a 2048-point transform
    (two 32-frame blocks no longer fit in LDS); NT = 2, 7 and 8 stand for the shape here.
  * k_mel_banded<2, 1> and <2, 2>: BNHIP_MEL_VARIANT experiments, process-wide, out of scope."""
from dataclasses import dataclass, field

import numpy as np

from birdnet_go_amd import synth_model as sm

S = sm.SpecConfig
NYQ = 24000.0

_BACKBONE = dict(stem=8, blocks=((1, 3, 1, 8, 1), (6, 3, 2, 12, 1)), top=16, n_classes=5, name="fe_case")


@dataclass
class Case:
    name: str
    cfg: sm.SynthConfig
    n_clips: int                     # clips of the GPU run (the CPU tests of the gate take N_CPU)
    steps: list                      # names of the plan's front-end steps, in order
    reaches: str                     # the kernel form(s) the case is in the table for
    env: dict = field(default_factory=dict)
    eng: dict = field(default_factory=dict)
    eps_t: float = 2.0 ** -53
    fpw: int = 1                     # frames per wave of k_stft_bins at n_clips (launch_stft_bins' rule, restated in the GPU test)
    nb: tuple = ()                   # needed bins per channel the case was built for (asserted from the mel constant)
    amp: float = 0.5                 # amplitude of the special clips' tones (the constant clip: half of it)
    twice: bool = False              # run the call twice on the engine (the parts kernel's counter must reset)


N_CPU = 10


def _cfg(specs, F, n_mels=32, extra=0, sample_rate=48000, **kw):
    pad = kw.get("pad", (0, 0))
    n = specs[0].frame_length + (F - 1) * specs[0].frame_step + extra - pad[0] - pad[1]
    base = dict(_BACKBONE)
    base.update(n_samples=n, sample_rate=sample_rate, specs=tuple(specs), n_mels=n_mels, seed=4242)
    base.update(kw)
    return sm.SynthConfig(**base)


def _steps(cfg, path, tail="banded"):
    """Names of the front-end steps the planner is expected to emit."""
    nch = len(cfg.specs)
    out = ["clip_minmax"] if cfg.normalize else []
    if path == "gemm":
        return out + [f"melspec{c}" for c in range(nch)]
    if cfg.normalize:
        out.append("normalize")
    if tail == "fused":
        return out + [f"stft{c}+mel" for c in range(nch)]
    out += [f"stft{c}" for c in range(nch)]
    c = 0
    while c < nch:
        pair = c + 1 < nch and c % 2 == 0
        sfx = f"{c}+{c + 1}" if pair else f"{c}"
        if tail == "dense":
            out += [f"mel{c}"] + ([f"mel{c + 1}"] if pair else []) + ["melspec" + sfx]
        else:
            out.append("melband" + sfx)
        c += 2 if pair else 1
    return out


_TAIL_ENV = {"banded": {}, "dense": {"BNHIP_NO_MEL_BANDED": "1"}, "fused": {"BNHIP_FUSE_MEL": "1"}}


def _variant(mode):
    """The two graph families: v2.4 (real part, normalised, power law, [mel, time]) and Perch-style (magnitude, raw, log, time-major)."""
    if mode == "real":
        return dict(complex_mode="real")
    return dict(complex_mode="abs", normalize=False, compress="log", time_major=True)


def _fft_matrix():
    """P = 4, 8, 16 x {real, magnitude} x {banded, dense GEMM + k_mel_finish, fused epilogue}; the frame is as long as the transform
    (512), 5/8 of it (1024) and half of it (2048); 12 frames, the last one ending at the clip's last sample."""
    geo = {512: S(512, 94, 200.0, 9000.0), 1024: S(640, 160, 300.0, 12000.0, 1024), 2048: S(1024, 278, 0.0, 3000.0, 2048)}
    out = []
    for N, sp in geo.items():
        for mode in ("real", "abs"):
            for tail in ("banded", "dense", "fused"):
                cfg = _cfg([sp], 12, **_variant(mode))
                mel = {"banded": "k_mel_banded<1>", "dense": "k_pw_gemm + k_mel_finish<1>", "fused": "MEL epilogue"}[tail]
                out.append(Case(f"fft{N}_{mode}_{tail}", cfg, 12, _steps(cfg, "fft", tail),
                                f"k_stft_bins<{N // 128}, {'MEL' if tail == 'fused' else 'bins'}, double> {mode}; {mel}", env=_TAIL_ENV[tail]))
    return out


def _fft_geometry():
    out = []
    cfg = _cfg([S(512, 94, 200.0, 9000.0)], 5, extra=40, complex_mode="abs")
    out.append(Case("fft512_F5", cfg, 12, _steps(cfg, "fft"), "F < 8: one partly filled block of k_stft_bins<4> and of k_mel_banded; clip longer than its last frame"))
    cfg = _cfg([S(510, 94, 200.0, 9000.0, 512)], 12)
    out.append(Case("fft512_Lm2", cfg, 12, _steps(cfg, "fft"), "L = N - 2: the window tail inside the last chunk"))
    cfg = _cfg([S(1022, 160, 300.0, 12000.0, 1024)], 12, **_variant("abs"))
    out.append(Case("fft1024_Lm2", cfg, 12, _steps(cfg, "fft"), "L = N - 2 at P = 8"))
    cfg = _cfg([S(1280, 278, 0.0, 3000.0, 2048)], 12, complex_mode="abs")
    out.append(Case("fft2048_L58", cfg, 12, _steps(cfg, "fft"), "L = 5N/8 at P = 16: the 128 n1 < L chunk guards"))
    cfg = _cfg([S(256, 94, 200.0, 9000.0, 512)], 12, **_variant("abs"))
    out.append(Case("fft512_Lhalf", cfg, 12, _steps(cfg, "fft"), "L = N/2 at P = 4"))
    cfg = _cfg([S(512, 95, 200.0, 9000.0)], 12)
    out.append(Case("fft512_oddhop", cfg, 12, _steps(cfg, "fft"), "odd hop: every second frame takes the scalar sample fetch"))
    for name, pad in (("pad7_13", (7, 13)), ("padhop_0", (94, 0)), ("pad0_Lhalf", (0, 256))):
        kw = _variant("abs") if name != "padhop_0" else dict(complex_mode="real", compress="log")
        cfg = _cfg([S(512, 94, 200.0, 9000.0)], 12, pad=pad, **kw)
        out.append(Case("fft512_" + name, cfg, 12, _steps(cfg, "fft"), f"clip PAD {pad}: frames before sample 0 / past the clip end (bounds-checked fetch)"))
    cfg = _cfg([S(500, 125, 200.0, 9000.0, 512)], 12, complex_mode="abs")
    assert cfg.n_samples % 2 == 1
    out.append(Case("fft512_oddclip", cfg, 12, _steps(cfg, "fft"), "odd n_samples (1875): every second clip is 4-byte aligned under the packed float2 fetch; scalar min/max"))
    # frames per wave above 1, by batch size: 360 frames of a 512-point transform
    cfg = _cfg([S(512, 16, 200.0, 9000.0)], 360, complex_mode="abs")
    out.append(Case("fft512_fpw2", cfg, 8, _steps(cfg, "fft"), "fpw = 2 (F n = 2880): the frame loop's prefetch, f_end clamp in the last block", fpw=2))
    cfg = _cfg([S(512, 17, 200.0, 9000.0)], 360, **_variant("abs"))
    out.append(Case("fft512_fpw16_oddhop", cfg, 87, _steps(cfg, "fft"), "fpw = 16 (F n = 31320), odd hop, odd n_samples", fpw=16))
    return out


def _fft_wide_banks():
    """Needed bins around and beyond 512; with the fused epilogue requested the plan must fall back to the separate mel step."""
    out = []
    for name, N, fmax, nb in (("fft1024_nb511", 1024, NYQ, 511), ("fft1024_nb512", 1024, NYQ * 1.04, 512), ("fft2048_nb1023", 2048, NYQ, 1023)):
        for fuse in (False, True):
            cfg = _cfg([S(N, 320, 0.0, fmax)], 9, **(_variant("abs") if N == 1024 else dict(complex_mode="abs")))
            out.append(Case(name + ("_fuse_asked" if fuse else ""), cfg, 12, _steps(cfg, "fft"),
                            f"{nb} needed bins" + (": the loop beyond 512 bins" if nb > 512 else ": the last register bin row full")
                            + ("; BNHIP_FUSE_MEL falls back to k_mel_banded (more than 256 quads or nbp > 512)" if fuse else ""),
                            env=_TAIL_ENV["fused"] if fuse else {}, nb=(nb,)))
    return out


PRUNE_BANKS = (("v24_0_3k", 0.0, 3000.0), ("high_15_20k", 15000.0, 20000.0), ("mid_9_15k", 9000.0, 15000.0), ("narrow_1k7_2k8", 1700.0, 2800.0))


def _fft_prune():
    """2048-point banks that differ in the closing stage's mask (run with BNHIP_STFT_PRUNE 1 and 0 by the GPU test); the narrow one
    needs bins 73..119 and their mirrors only: passes 0 and 3 of the closing stage are pruned whole."""
    out = []
    for name, lo, hi in PRUNE_BANKS:
        cfg = _cfg([S(2048, 278, lo, hi)], 12, n_mels=16 if name.startswith("narrow") else 32, complex_mode="abs" if name.startswith("mid") else "real")
        out.append(Case("prune_" + name, cfg, 12, _steps(cfg, "fft"), f"k_stft_bins<16> output pruning, bank {lo:.0f}-{hi:.0f} Hz"))
    return out


def _fft_f32():
    geo = {512: S(320, 160, 60.0, 16000.0, 512), 1024: S(640, 320, 60.0, 16000.0, 1024), 2048: S(2048, 278, 0.0, 3000.0, 2048)}
    out = []
    for N, sp in geo.items():
        cfg = _cfg([sp], 12, sample_rate=32000 if N < 2048 else 48000, pad=(80, 80) if N < 2048 else (0, 0), **_variant("abs"))
        out.append(Case(f"f32_fft{N}", cfg, 12, _steps(cfg, "fft"), f"k_stft_bins<{N // 128}, bins, float>: the fp32 transform of a bf16 engine, log compression",
                        eng=dict(precision="bf16"), eps_t=2.0 ** -24, amp=0.05))
    return out


def _fft_channels():
    a, b, c = S(512, 94, 0.0, 3000.0), S(512, 94, 500.0, 15000.0), S(512, 94, 200.0, 8000.0)
    b8 = S(512, 94, 500.0, 15000.0, 1024)
    out = []
    for name, specs, n_mels, kw, tail in (
            ("ch1_mel16", [a], 16, _variant("real"), "banded"),
            ("ch2_tm_mel96", [a, b], 96, _variant("abs"), "banded"),
            ("ch3_mel97", [a, b, c], 97, _variant("real"), "banded"),
            ("ch2_mel128", [a, b8], 128, dict(complex_mode="abs"), "banded"),
            ("ch3_tm_mel32", [a, b, c], 32, _variant("abs"), "banded"),
            ("ch2_dense", [a, b], 32, _variant("real"), "dense"),
            ("ch3_tm_dense", [a, b, c], 33, _variant("abs"), "dense"),
            ("ch2_fused", [a, b], 32, _variant("real"), "fused")):
        cfg = _cfg(specs, 21, n_mels=n_mels, **kw)
        nch = len(specs)
        forms = {"banded": "k_mel_banded<2>" if nch > 1 else "k_mel_banded<1>", "dense": "k_mel_finish<2>" if nch > 1 else "k_mel_finish<1>", "fused": "MEL epilogue"}[tail]
        if nch == 3:
            forms += " + <1> (stride-3 stores)"
        out.append(Case(name, cfg, 12, _steps(cfg, "fft", tail), f"{nch} channel(s), {'time-major' if cfg.time_major else '[mel, time]'}, n_mels {n_mels}"
                        f"{' (256-thread block)' if n_mels > 96 else ''}: {forms}", env=_TAIL_ENV[tail]))
    return out


def _gemm():
    """The folded-GEMM kernel: fft_length 256 / 384 (the FFT path does not take them), or frontend_fft = 0."""
    out = []
    for n_mels, NT, WN in ((16, 1, 1), (17, 2, 2), (48, 3, 1), (64, 4, 2), (80, 5, 1), (96, 6, 2), (112, 7, 1), (128, 8, 2)):
        sp = S(384, 96, 100.0, 12000.0) if NT == 3 else S(256, 96, 100.0, 12000.0)
        cfg = _cfg([sp], 11 if NT == 4 else 21, n_mels=n_mels, extra=(96 if NT == 3 else 32) if NT % 2 else 0)      # (odd NT: the clip runs on past its last frame)
        out.append(Case(f"gemm_nt{NT}", cfg, 12, _steps(cfg, "gemm"), f"k_frontend<{NT}, {WN}, 32, 16>, fft_length {sp.frame_length}, F = {11 if NT == 4 else 21}"))
    cfg = _cfg([S(2048, 278, 0.0, 3000.0)], 70, n_mels=128)
    out.append(Case("gemm_nt8_ft64", cfg, 12, _steps(cfg, "gemm"), "k_frontend<8, 2, 64, 32>: two frame tiles, the second partial", eng=dict(frontend_fft=0)))
    cfg = _cfg([S(2048, 278, 500.0, 15000.0)], 21, n_mels=112)
    out.append(Case("gemm_nt7_ft64", cfg, 12, _steps(cfg, "gemm"), "k_frontend<7, 1, 64, 32>", eng=dict(frontend_fft=0)))
    cfg = _cfg([S(2048, 450, 0.0, 3000.0)], 20, n_mels=32)
    out.append(Case("gemm_nt2_ft64", cfg, 12, _steps(cfg, "gemm"), "k_frontend<2, 2, 64, 32> (hop 450: two 32-frame blocks do not fit)", eng=dict(frontend_fft=0)))
    cfg = _cfg([S(512, 94, 0.0, 3000.0), S(512, 94, 500.0, 15000.0)], 21, n_mels=40)
    out.append(Case("gemm_2ch_fft0", cfg, 12, _steps(cfg, "gemm"), "k_frontend<3, 1, 32, 16> twice: two channels into one image, frontend_fft = 0", eng=dict(frontend_fft=0)))
    cfg = _cfg([S(200, 100, 100.0, 12000.0, 256)], 21, n_mels=24)
    out.append(Case("gemm_Lshort", cfg, 12, _steps(cfg, "gemm"), "k_frontend<2, 2, 32, 16>: frame (200) shorter than the transform (256)"))
    cfg = _cfg([S(250, 125, 100.0, 12000.0, 256)], 12, n_mels=24)
    assert cfg.n_samples % 2 == 1
    out.append(Case("gemm_oddclip", cfg, 12, _steps(cfg, "gemm"), "k_frontend scalar staging: odd n_samples (1625), clips 4-byte aligned"))
    return out


def _minmax():
    out = []
    cfg = _cfg([S(512, 92, 200.0, 9000.0)], 12)
    assert cfg.n_samples % 4 == 0
    out.append(Case("minmax_vec_resident", cfg, 20, _steps(cfg, "fft"), "k_clip_minmax float4 path (n_samples % 4 == 0); 20 clips: k_clip_norm_resident when switched on"))
    cfg = _cfg([S(512, 5912, 200.0, 9000.0)], 12)
    assert cfg.n_samples % 4 == 0 and cfg.n_samples >= 65536
    out.append(Case("minmax_parts", cfg, 12, _steps(cfg, "fft"), "k_clip_minmax_parts (12 clips of 65 544 samples), called twice: the arrival counter resets", twice=True))
    return out


CASES = _fft_matrix() + _fft_geometry() + _fft_wide_banks() + _fft_prune() + _fft_f32() + _fft_channels() + _gemm() + _minmax()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def clips(case, n):
    """(x [n, n_samples], live): synth_clips material with the special clips at fixed places; `live` lists the clips whose every
    frame carries broadband material (the ones a structural error must show on).
      1 all zero            2 constant (range 0: eps alone divides)      3 extremes at the first and the last sample
      4 zero first half     5 one full-scale impulse in the last frame   6 tone exactly on a needed bin of channel 0
      7 tone exactly on a bin channel 0's bank does not read (DC when it reads all the others)"""
    from feref import model_consts, needed_bins
    cfg = case.cfg
    assert n >= 8
    ns, sp = cfg.n_samples, cfg.specs[0]
    N = sp.fft_length or sp.frame_length
    x = sm.synth_clips(n, ns, cfg.sample_rate, first=3)
    x[1] = 0.0
    x[2] = 0.5 * case.amp
    x[3, 0], x[3, -1] = -1.5, 1.75
    x[4, :ns // 2] = 0.0
    x[5] = 0.0
    x[5, ns - 1 - min(sp.frame_length // 3, ns - 1)] = 1.0
    need = needed_bins(model_consts(model(case), 1)[0][1])
    k_in = int(need[need.size // 2])
    rest = np.setdiff1d(np.arange(N // 2 + 1), need)
    k_out = int(rest[rest.size // 2])
    t = np.arange(ns, dtype=np.float64)
    x[6] = (case.amp * np.cos(2.0 * np.pi * k_in * t / N)).astype(np.float32)
    x[7] = (case.amp * np.cos(2.0 * np.pi * k_out * t / N)).astype(np.float32)
    # extremes in the first and in the last quad of the clip (first / last part of the parts kernel) on a material clip
    if n > 8:
        x[8, 1], x[8, -2] = -1.25, 1.125
    live = [0, 3] + list(range(8, n))
    return x, live


_models = {}


def model(case):
    if case.name not in _models:
        _models[case.name] = sm.build_model(case.cfg)
    return _models[case.name]
