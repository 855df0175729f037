"""Plain-numpy reference of the mel front end at the tensors its kernels write, with a derived tolerance per bin and an allowed
interval per spectrogram pixel.  Independent of oracle/interp.py: the graph's constants (window, mel matrix) are read from the
model file by name, everything else comes from the SynthConfig the model was built from.

Graph semantics, exact where the graph is exact:
  * normalise and window in float32, one IEEE operation per graph op, in the graph's order: REDUCE_MIN, SUB, REDUCE_MAX, ADD eps,
    DIV, SUB 0.5, MUL 2, then PAD, framing, MUL by the Hann constant.  numpy float32 is what the device must produce bit for bit
    (`mm`, `xn`), and the windowed frame is rounded to float32 as TFLite rounds it (an fp64 interpreter does not).
  * zero-pad to fft_length, real DFT in float64; real part or magnitude narrowed to float32: the bins x^.
  * mel sum v over the fp32 bins in float64; compression |v|^(2 p2) or log_scale * ln(max(v, log_floor)) in float64.
  * layout as the graph's: REVERSE_V2 + TRANSPOSE ([mel, time]) or time-major; channels last.

The gate (derived, not measured; eps_T = 2^-53 for the fp64 transform, 2^-24 for the fp32 one; N = fft_length; A_f = sum_n |frame_f[n]|):
  bins      tol[f, k] = (2^-23 + c_abs) |X_k| + eps_T log2(N) A_f     (one ulp of the narrowed bin - hypotf's own ulp for the
                                                                       magnitude - plus the standard FFT round-off bound;
                                                                       measured against the UNROUNDED fp64 value)
  mel       tau[f, m] = sum_k |w[m, k]| (2^-24 (span_m + 3) |x^_k| + (2^-23 + c_abs) |x^_k| + eps_T log2(N) A_f)
                                                                      (span_m = the band's non-zero weights: fp32 products and
                                                                       sums in any order; then the bin's own tolerance)
  c_abs = 2^-23 for the magnitude graph, 0 for the real-part graph.  COMPLEX_ABS works on complex64: BOTH components are narrowed
  to fp32 before the magnitude is taken - d|X| <= sqrt(dr^2 + di^2) <= 2^-24 |X| - and the device's hypotf is
  sqrt(fl(a a) + b b) by fma on the hardware root: the product's and the fma's roundings are 2 x 2^-24 of the sum, halved by the
  root, 2^-24; then the root's own ulp, 2^-23.  2^-24 + 2^-24 + 2^-23 = 2^-22 in all.  (The device runs showed both: magnitude
  bins at 1.27 of a tolerance of one ulp for narrowing and hypotf together, and at 1.05 - one bin of 2.9 million - with hypotf
  taken as one ulp on top of the narrowing.  The real part, a single narrowing, measures 0.50 of its 2^-23.)
  pixel     [lo, hi] = range of the compression over [v - tau, v + tau] (lower end 0 when the interval contains 0 under the
            power law), both ends widened relatively by 2^-21 (1 + |log2 |hi||): one ulp each of the hardware log2 and exp2 (or
            powf) under the exponent, the square, the narrowing and the store.
With `half_out` (an image stored as bf16) half a bf16 ulp of the end's magnitude, 2^-9 |end|, is added to each end.
Every pixel is checked; none is left out."""
from dataclasses import dataclass

import numpy as np

from oracle.tflite_reader import read_model

F32 = np.float32
EPS_T64, EPS_T32 = 2.0 ** -53, 2.0 ** -24


def model_consts(model, n_channels):
    """[(window f32 [L], mel f32 [n_mels, n_bins])] per channel, from the model file's named constants."""
    m = model if hasattr(model, "tensors") else read_model(model)
    by_name = {t.name: t for t in m.tensors if t.data is not None}
    return [(np.asarray(by_name[f"MEL{c}/hann"].data, F32).reshape(-1), np.asarray(by_name[f"MEL{c}/mel"].data, F32)) for c in range(n_channels)]


def needed_bins(mel):
    """The planner's rule: a DFT bin (column of the [n_mels, n_bins] matrix) with any non-zero weight."""
    return np.flatnonzero((np.asarray(mel) != 0).any(axis=0))


def band_spans(mel, bins):
    """[lo, hi) of each band's non-zero columns in the needed-bins numbering (0, 0 for an empty band)."""
    w = np.asarray(mel)[:, bins] != 0
    out = []
    for row in w:
        nz = np.flatnonzero(row)
        out.append((int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 0))
    return out


def mel_quads(mel, bins):
    """The fused epilogue's table size (stft_mel_table): aligned quads of four needed bins each band touches, summed."""
    return sum(((hi + 3) >> 2) - (lo >> 2) if hi > lo else 0 for lo, hi in band_spans(mel, bins))


def normalise(x, eps=1e-6):
    """(mm [B, 2], xn [B, n]) in float32, operation for operation; mm = (min, fl(max - min) + eps)."""
    x = np.asarray(x, F32)
    mn = x.min(axis=1, keepdims=True)
    s1 = x - mn
    mx = s1.max(axis=1, keepdims=True)
    dn = mx + F32(eps)
    nm = s1 / dn
    n2 = nm - F32(0.5)
    xn = n2 * F32(2.0)
    assert xn.dtype == F32
    return np.concatenate([mn, dn], axis=1), xn


def frames_of(xp, L, hop, F, last_shift=0):
    """[B, F, L] sliding windows of the padded clip; last_shift moves the last frame's start (a structural error for the gate's own test)."""
    idx = np.arange(F)[:, None] * hop + np.arange(L)[None, :]
    if last_shift:
        idx[-1] += last_shift
    return xp[:, idx]


@dataclass
class ChannelRef:
    frames: np.ndarray     # [B, F, L] float32, windowed (rounded to fp32)
    X: np.ndarray          # [B, F, n_bins] float64: the exact transform's real part or magnitude, not narrowed
    bins: np.ndarray       # [B, F, n_bins] float32: real part or magnitude, narrowed
    bin_tol: np.ndarray    # [B, F, n_bins] float64
    v: np.ndarray          # [B, F, n_mels] float64, graph order of the mel axis
    tau: np.ndarray        # [B, F, n_mels] float64
    needed: np.ndarray     # needed bin indices
    win_sum: float = 0.0   # sum of the window's taps
    mel: np.ndarray = None # [n_mels, n_bins] float32 as used


@dataclass
class FrontRef:
    mm: np.ndarray         # [B, 2] float32 or None (raw front end)
    xn: np.ndarray         # [B, n_samples] float32 (the clip itself when the front end is raw)
    chans: list
    mid: np.ndarray        # [B, H, W, C] float64 image: the compression of v
    lo: np.ndarray
    hi: np.ndarray


def compress(cfg, v):
    v = np.asarray(v, np.float64)
    if cfg.compress == "pow":
        e = 2.0 * float(F32(1.0 / (1.0 + np.exp(cfg.mag_scale))))
        return np.abs(v) ** e
    return float(F32(cfg.log_scale)) * np.log(np.maximum(v, float(F32(cfg.log_floor))))


def pixel_interval(cfg, v, tau, half_out=False):
    """Allowed [lo, hi] of the compressed value for a mel sum within tau of v (see the module docstring)."""
    a, b = v - tau, v + tau
    if cfg.compress == "pow":
        ca, cb = compress(cfg, a), compress(cfg, b)
        hi = np.maximum(ca, cb)
        lo = np.where((a <= 0) & (b >= 0), 0.0, np.minimum(ca, cb))
    else:
        lo, hi = compress(cfg, a), compress(cfg, b)
    mag = np.abs(hi)
    with np.errstate(divide="ignore"):
        w = np.where(mag > 0, 2.0 ** -21 * (1.0 + np.abs(np.log2(np.where(mag > 0, mag, 1.0)))), 0.0)
    extra = 2.0 ** -9 if half_out else 0.0
    return lo - (w + extra) * np.abs(lo), hi + (w + extra) * np.abs(hi)


def layout(cfg, per_channel):
    """[B, F, n_mels] per channel (graph order of the mel axis) -> the image [B, H, W, C]."""
    out = []
    for a in per_channel:
        out.append(a if cfg.time_major else np.flip(a, axis=2).transpose(0, 2, 1))
    return np.stack(out, axis=-1)


def front_end(cfg, model, x, eps_t=EPS_T64, half_out=False, mutate=None):
    """The reference of every front-end tensor for clips x [B, n_samples].  `mutate` recomputes it with ONE deliberate structural
    error (the gate's own test): "last_frame_early", "window_tap", "band_shift", "bin_plus_one", "swap_channels",
    "repeat_frame", "mel_order"."""
    x = np.asarray(x, F32)
    consts = model_consts(model, len(cfg.specs))
    if cfg.normalize:
        mm, xn = normalise(x)
    else:
        mm, xn = None, x
    xp = np.pad(xn, [(0, 0), tuple(cfg.pad)])
    n_pad = xp.shape[1]
    chans = []
    for sp, (win, mel) in zip(cfg.specs, consts):
        L, hop, N = sp.frame_length, sp.frame_step, sp.fft_length or sp.frame_length
        F = 1 + (n_pad - L) // hop
        assert win.shape == (L,) and mel.shape == (cfg.n_mels, N // 2 + 1) and mel.dtype == F32
        if mutate == "window_tap":
            win = np.roll(win, 1)
        fr = frames_of(xp, L, hop, F, -1 if mutate == "last_frame_early" else 0) * win[None, None, :]
        assert fr.dtype == F32
        if mutate == "repeat_frame":
            fr = fr.copy(); fr[:, -1] = fr[:, -2]
        Xc = np.fft.rfft(fr.astype(np.float64), n=N, axis=-1)
        if mutate == "bin_plus_one":
            Xc = np.concatenate([Xc[..., 1:], Xc[..., :1]], axis=-1)
        bins = (Xc.real if cfg.complex_mode == "real" else np.abs(Xc)).astype(F32)
        need = needed_bins(mel)
        if mutate == "band_shift":
            mel = mel.copy(); mid = int((mel != 0).sum(axis=1).argmax()); mel[mid] = np.roll(mel[mid], 1)      # the widest band
        A = np.abs(fr.astype(np.float64)).sum(axis=-1)[..., None]
        fft_term = eps_t * np.log2(N) * A
        exact = Xc.real if cfg.complex_mode == "real" else np.abs(Xc)
        ulp1 = 2.0 ** -23 + (2.0 ** -23 if cfg.complex_mode == "abs" else 0.0)
        bin_tol = ulp1 * np.abs(exact) + fft_term
        w = np.abs(mel.astype(np.float64))
        span = (mel != 0).sum(axis=1).astype(np.float64)
        absb = np.abs(bins.astype(np.float64))
        v = bins.astype(np.float64) @ mel.astype(np.float64).T
        tau = (2.0 ** -24 * (span + 3.0) + ulp1)[None, None, :] * (absb @ w.T) + fft_term * w.sum(axis=1)[None, None, :]
        chans.append(ChannelRef(fr, exact, bins, bin_tol, v, tau, need, float(np.abs(win.astype(np.float64)).sum()), mel))
    order = list(range(len(chans)))
    if mutate == "swap_channels":
        order[0], order[1] = order[1], order[0]
    flip = (lambda a: np.flip(a, axis=2)) if mutate == "mel_order" else (lambda a: a)
    vs, taus = [flip(chans[i].v) for i in order], [flip(chans[i].tau) for i in order]
    mid = layout(cfg, [compress(cfg, v) for v in vs])
    los, his = zip(*(pixel_interval(cfg, v, t, half_out) for v, t in zip(vs, taus)))
    return FrontRef(mm, xn, chans, mid, layout(cfg, los), layout(cfg, his))


def check_image(got, ref):
    """(worst excess / interval width, number of pixels outside, excess array) of an image against the intervals.  A pixel inside
    has excess 0 (ratio 0); a pixel outside a zero-width interval has ratio inf."""
    got = np.asarray(got, np.float64).reshape(ref.lo.shape)
    excess = np.maximum(np.maximum(ref.lo - got, got - ref.hi), 0.0)
    excess = np.where(np.isfinite(got), excess, np.inf)
    width = ref.hi - ref.lo
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(excess > 0, excess / width, 0.0)
    return float(ratio.max()), int((excess > 0).sum()), excess


def check_bins(got, ch, nbp):
    """got [B, F, nbp] device bins tensor of one channel: (worst |error| / tolerance over the needed bins, number of non-zero
    padding columns)."""
    nb = ch.needed.size
    got = np.asarray(got).reshape(ch.bins.shape[0], ch.bins.shape[1], nbp)
    err = np.abs(got[..., :nb].astype(np.float64) - ch.X[..., ch.needed])
    tol = ch.bin_tol[..., ch.needed]
    bad = ~np.isfinite(got[..., :nb])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / tol, 0.0)
    ratio = np.where(bad, np.inf, ratio)
    pad = got[..., nb:]
    return float(ratio.max()) if ratio.size else 0.0, int((pad != 0).sum() + np.signbit(pad).sum())
