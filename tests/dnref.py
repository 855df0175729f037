"""Float64 restatement of the denoise spec (DESIGN.md §9 "Denoise") in numpy: what bnhip_denoise_* is pinned to.

Not a restatement of FFmpeg's afftdn: FFmpeg is not in the reference's tree, the spec is this project's own.  Kept from the
reference (internal/audiocore/ffmpeg/process.go:181-203): the two parameters nr / nf, the presets, the validation rules.
Everything below follows the spec line by line; `denoise` returns the value before rounding, `quant` rounds it."""
import numpy as np

PRESETS = {"light": (6, -30), "medium": (12, -40), "heavy": (20, -50)}       # denoisePresets (process.go:182-186)
TOL = 1e-6                                                                   # LSB: how near a rounding tie a sample is excused


def hann(N):
    """Periodic Hann."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)


def frame_count(n, N):
    h = N // 4
    return -(-n // h) + 3


def g_min(nr_db):
    return 10.0 ** (-nr_db / 20.0)


def denoise(pcm, N, nr_db, nf_db):
    """One clip: int16 [n] -> float64 [n], v of the spec (before rounding)."""
    pcm = np.asarray(pcm)
    assert pcm.dtype == np.int16 and pcm.ndim == 1 and pcm.size >= 1
    n, h = pcm.size, N // 4
    M = frame_count(n, N)
    w = hann(N)
    # x = 0 outside [0, n): 3 hops in front, and up to the end of the last frame behind
    xp = np.zeros((M + 3) * h)
    xp[3 * h:3 * h + n] = pcm.astype(np.float64) / 32768.0
    fr = xp[np.arange(M)[:, None] * h + np.arange(N)[None, :]] * w            # frame m starts at (m - 3) h
    X = np.fft.rfft(fr, axis=-1)
    P = X.real ** 2 + X.imag ** 2
    Pm = np.concatenate([P[:, 1:2], P[:, :-1]], axis=1)                       # P[k - 1], mirrored at 0
    Pp = np.concatenate([P[:, 1:], P[:, -2:-1]], axis=1)                      # P[k + 1], mirrored at N/2
    Pb = ((Pm + Pp) + 2.0 * P) * 0.25
    Nz = 10.0 ** (nf_db / 10.0) * (3.0 * N / 8.0)
    gm = g_min(nr_db)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(Pb > 0.0, np.maximum(gm, 1.0 - Nz / Pb), gm)
    y = np.fft.irfft(g * X, n=N, axis=-1) * w
    acc = np.zeros((M + 3) * h)
    for m in range(M):                                                        # frame order
        acc[m * h:m * h + N] += y[m]
    return 32768.0 * (2.0 / 3.0) * acc[3 * h:3 * h + n]


def quant(v):
    """Round half away from zero, saturate to int16 (pcmgain.ApplyInt16's rule)."""
    v = np.asarray(v, np.float64)
    return np.clip(np.sign(v) * np.floor(np.abs(v) + 0.5), -32768.0, 32767.0).astype(np.int16)


def denoise_pcm16(clips, N, nr_db, nf_db):
    """int16 [B, n] -> (int16 [B, n], v float64 [B, n])."""
    clips = np.atleast_2d(np.asarray(clips))
    v = np.stack([denoise(c, N, nr_db, nf_db) for c in clips])
    return quant(v), v


def excused(v, tol=TOL):
    """Samples whose |v| + 0.5 lies within tol of an integer: a rounding tie that float64 evaluation order may break either way."""
    t = np.abs(v) + 0.5
    return np.abs(t - np.round(t)) <= tol


def tie_share(v):
    return float(excused(v).mean())


def check_cap(v, cap=1e-4):
    """The condition on a case's inputs, over all of its clips together."""
    share = tie_share(v)
    assert share <= cap, f"restatement: {share:.3g} of the samples sit on a rounding tie (cap {cap}): the case needs another seed"
    return share


def compare(dev, clips, N, nr_db, nf_db, cap=1e-4, restated=None):
    """The acceptance rule: equal at every sample, except that an excused sample may differ by 1 LSB; the excused share of the case
    is capped, asserted on the restatement before the device output is looked at.  clips, dev: int16 [B, n]; restated: what
    denoise_pcm16 gave for these arguments, where a caller has it already."""
    ref, v = restated if restated is not None else denoise_pcm16(clips, N, nr_db, nf_db)
    share = check_cap(v, cap)
    ex = excused(v)
    dev = np.asarray(dev)
    assert dev.shape == ref.shape and dev.dtype == np.int16
    diff = np.abs(dev.astype(np.int32) - ref.astype(np.int32))
    bad = (diff > 0) & ~(ex & (diff <= 1))
    assert not bad.any(), (f"{int(bad.sum())} samples differ (max {int(diff.max())}); first at {tuple(np.argwhere(bad)[0])}: "
                           f"device {dev[bad][0]}, restatement {ref[bad][0]}, v {v[bad][0]!r}")
    return share
