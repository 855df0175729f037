"""The images of the PNG tests (test_png_ref.py on the CPU, test_png.py on the device), built once and never written.

A case is (images uint8 [n, H, W], the forms its first image's bands must take, or None where they are mixed).  A band is
R = ceil(16384 / (W + 1)) rows, so a band that is not an image's last holds at least 16384 bytes: the cases with several bands use
narrow, tall images."""
import functools

import numpy as np

import pngref
import specref

Z, HU, ST = pngref.ZERO, pngref.HUFFMAN, pngref.STORED


def _ro(a):
    a = np.ascontiguousarray(a, np.uint8)
    a.setflags(write=False)
    return a


def palette():
    pal = np.random.default_rng(1948).integers(0, 256, (256, 3)).astype(np.uint8)
    pal.setflags(write=False)
    return pal


def skewed(rng, shape, values=256):
    """Bytes with a geometric-like distribution over `values` values: compressible, every value possible."""
    v = np.minimum(rng.geometric(0.08, shape) - 1, values - 1)
    return v.astype(np.uint8)


def fibonacci_image():
    """56 x 192 pixels whose band of 192 * 57 = 10944 bytes has Fibonacci counts F(2)..F(19) = 1, 2, 3, 5, .. 4181 over 18 byte values
    (their sum is F(21) - 2 = 10944); value 0 takes 233: the 192 filter bytes and 41 pixels.  With the end-of-block symbol's 1 in
    front, every Huffman merge joins the running sum to the next leaf: depth 18."""
    f = [1, 2]
    while len(f) < 18:
        f.append(f[-1] + f[-2])
    values = [13 * k + 5 for k in range(18)]
    values[f.index(233)] = 0
    px = np.concatenate([np.full(c - (192 if v == 0 else 0), v, np.uint8) for v, c in zip(values, f)])
    assert px.size == 56 * 192
    np.random.default_rng(5).shuffle(px)
    return px.reshape(192, 56)


def rendered_image():
    """A real image at 258 x 129: a chirp over noise, rendered by the spectrogram's restatement."""
    n, rate = 24000, 24000
    rng = np.random.default_rng(11)
    t = np.arange(n) / rate
    x = 12000.0 * np.sin(2.0 * np.pi * (300.0 * t + 5000.0 * t * t)) + rng.integers(-300, 301, n)
    return specref.render_pcm16(np.round(x).astype(np.int16), 258, 129)


def mixed_batch(count=300, w=24, h=20):
    """Tiny images, by i mod 3: all zero (ZERO), two values (HUFFMAN), uniform random bytes (STORED)."""
    rng = np.random.default_rng(300)
    out = np.zeros((count, h, w), np.uint8)
    for i in range(count):
        if i % 3 == 1:
            out[i] = 9 * (rng.random((h, w)) < 0.2)
        elif i % 3 == 2:
            out[i] = rng.integers(0, 256, (h, w))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(2024)
    zeros = lambda h, w: np.zeros((1, h, w), np.uint8)
    three = skewed(rng, (3072, 15), 40)                                      # R = 1024
    three[1024:2048] = 0
    every = skewed(rng, (64, 64))
    every.reshape(-1)[:256] = np.arange(256)
    c = {
        "1x1": (np.full((1, 1, 1), 7, np.uint8), [ST]),
        "1xH": (skewed(rng, (1, 37, 1)), [HU]),
        "Wx1": (skewed(rng, (1, 1, 300), 12), [HU]),
        "one_band": (skewed(rng, (1, 2048, 7), 40), [HU]),                  # R = 2048: exactly one band
        "two_bands": (skewed(rng, (1, 4096, 7), 40), [HU, HU]),
        "short_last_band": (skewed(rng, (1, 2050, 7), 40), [HU, ST]),       # the last band is 2 rows, 16 bytes
        "zero_mod258_0": (zeros(37, 6), [Z]),                               # n = 259
        "zero_mod258_1": (zeros(65, 3), [Z]),                               # n = 260
        "zero_mod258_2": (zeros(29, 8), [Z]),                               # n = 261
        "zero_mod258_3": (zeros(131, 1), [Z]),                              # n = 262: the shortest match
        "zero_mod258_3_twice": (zeros(13, 39), [Z]),                        # n = 520
        "zero_extra_bits": (zeros(1, 100), [Z]),                            # n = 101: one match of 100, base 99 and 4 extra bits
        "zero_n2": (zeros(1, 1), [Z]),                                      # n - 1 = 1: one literal more
        "zero_n3": (zeros(1, 2), [Z]),                                      # n - 1 = 2: two literals more
        "zero_long": (zeros(300, 50), [Z]),                                 # n = 15300: 59 matches of 258 and one of 77
        "zero_between": (three[None], [HU, Z, HU]),
        "two_values": (9 * (rng.random((1, 40, 50)) < 0.3), [HU]),
        "all_256": (every[None], [HU]),
        "stored_final": (rng.integers(0, 256, (1, 50, 100)), [ST]),
        "stored_both": (rng.integers(0, 256, (1, 256, 127)), [ST, ST]),     # R = 128: a non-final and a final band of 16384
        "fibonacci": (fibonacci_image()[None], [HU]),
        "batch300": (mixed_batch(), None),
        "rendered": (rendered_image()[None], [HU, HU, HU]),        # R = 64
        "three_images": (np.stack([skewed(rng, (33, 45), 30), np.zeros((33, 45), np.uint8), rng.integers(0, 256, (33, 45))]), [HU]),
    }
    return {k: (_ro(v[0]), v[1]) for k, v in c.items()}


NAMES = ("1x1", "1xH", "Wx1", "one_band", "two_bands", "short_last_band", "zero_mod258_0", "zero_mod258_1", "zero_mod258_2",
         "zero_mod258_3", "zero_mod258_3_twice", "zero_extra_bits", "zero_n2", "zero_n3", "zero_long", "zero_between", "two_values",
         "all_256", "stored_final", "stored_both", "fibonacci", "batch300", "rendered", "three_images")


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (the restated streams back to back, offsets[n + 1]), computed once."""
    images, _ = cases()[name]
    return pngref.encode_batch(images, palette())
