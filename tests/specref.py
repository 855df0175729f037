"""Float64 restatement of the spectrogram rendering spec in numpy: what bnhip_spectrogram_* is pinned to.

Not a restatement of sox: sox is not in the reference's tree, the spec is this project's own.  Everything
below follows the spec line by line; `direct=True` evaluates the DFT as a matrix product instead of numpy's FFT (the two
agree on every pixel of the test inputs, which is what makes either usable as the yardstick)."""
import numpy as np


def fft_friendly_height(width):
    """generator.go:115-123: the smallest 2^k + 1 that is >= width // 2."""
    target = width // 2
    n = 1
    while n + 1 < target:
        n *= 2
    return n + 1


def hann(n):
    """Periodic Hann, the NULL-window default."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def frames_per_column(n, width, fft):
    return max(1, -(-n // (width * fft)))


def frame_centres(n, width, fft):
    """[width, K] sample index each frame is centred at (Python integers: no overflow)."""
    K = frames_per_column(n, width, fft)
    return np.array([[((2 * (c * K + k) + 1) * n) // (2 * K * width) for k in range(K)] for c in range(width)], np.int64)


def frame_powers(x, width, height, window=None, direct=False):
    """x: float64 [n] -> P_k [width, K, height]: (re^2 + im^2) (2 / sum w)^2 of every frame."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    N = 2 * (height - 1)
    w = hann(N) if window is None else np.asarray(window, np.float64)
    assert w.shape == (N,)
    m = frame_centres(n, width, N)
    idx = m[:, :, None] - N // 2 + np.arange(N)[None, None, :]
    inside = (idx >= 0) & (idx < n)
    fr = np.where(inside, x[np.clip(idx, 0, n - 1)], 0.0) * w
    if direct:
        b = np.arange(height)[:, None] * np.arange(N)[None, :]
        ang = -2.0 * np.pi * (b % N) / N
        X = fr @ (np.cos(ang) + 1j * np.sin(ang)).T
    else:
        X = np.fft.rfft(fr, axis=-1)
    scale = (2.0 / w.sum()) ** 2
    return (X.real ** 2 + X.imag ** 2) * scale


def level_value(P, top_db=0.0, range_db=100.0):
    """v of the spec (-inf where P = 0)."""
    with np.errstate(divide="ignore"):
        db = 10.0 * np.log10(P)
    return (db - top_db + range_db) / range_db * 255.0


def levels(v):
    out = np.floor(np.clip(v, 0.0, 255.0) + 0.5)
    out[~(v > 0.0)] = 0.0
    out[v >= 255.0] = 255.0
    return out.astype(np.uint8)


def column_power(x, width, height, window=None, direct=False):
    """P [width, height]: the K frame powers of a column summed in the order k = 0..K-1, divided by K."""
    Pk = frame_powers(x, width, height, window, direct)
    K = Pk.shape[1]
    s = np.zeros((width, height))
    for k in range(K):
        s = s + Pk[:, k, :]
    return s / K


def render(x, width, height, window=None, top_db=0.0, range_db=100.0, direct=False, with_v=False):
    """One clip -> uint8 [height, width] (row r = bin height - 1 - r); with_v: also v in the same layout."""
    P = column_power(x, width, height, window, direct)
    v = level_value(P, top_db, range_db)
    v = v.T[::-1]
    img = levels(v)
    return (img, v) if with_v else img


def render_pcm16(pcm, width, height, **kw):
    return render(np.asarray(pcm, np.int16).astype(np.float64) / 32768.0, width, height, **kw)


def excused(v, range_db=100.0, tol_db=1e-6):
    """Pixels whose v + 0.5 lies within tol_db (in level units: tol_db * 255 / range_db) of an integer: a rounding tie that
    float64 evaluation order may break either way."""
    with np.errstate(invalid="ignore"):
        t = v + 0.5
        d = np.abs(t - np.round(t))
        return np.isfinite(v) & (v > -1.0) & (v < 256.0) & (d <= tol_db * 255.0 / range_db)


def compare(dev, x, width, height, window=None, top_db=0.0, range_db=100.0, cap=1e-4):
    """The acceptance rule: equal at every pixel, except that an excused pixel may differ by 1; the excused share is capped
    (asserted on the restatement before the device image is looked at).  x: float64 [n]; dev: uint8 [height, width]."""
    ref, v = render(x, width, height, window, top_db, range_db, with_v=True)
    ex = excused(v, range_db)
    share = float(ex.mean())
    assert share <= cap, f"restatement: {share:.3g} of the pixels sit on a rounding tie (cap {cap})"
    dev = np.asarray(dev)
    assert dev.shape == ref.shape and dev.dtype == np.uint8
    diff = np.abs(dev.astype(np.int32) - ref.astype(np.int32))
    bad = (diff > 0) & ~(ex & (diff <= 1))
    assert not bad.any(), (f"{int(bad.sum())} pixels differ (max {int(diff.max())}); first at {tuple(np.argwhere(bad)[0])}: "
                           f"device {dev[bad][0]}, restatement {ref[bad][0]}, v {v[bad][0]!r}")
    return share
