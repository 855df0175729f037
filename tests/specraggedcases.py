"""The bursts of the ragged spectrogram tests (test_spectrogram_ragged_ref.py on the CPU, test_spectrogram_ragged.py on the device):
lists of int16 clips of unequal lengths at 24 kHz, every length the smallest at which a per-clip mechanism of k_spectrogram can go
wrong.  Signals cycle through test_spectrogram.signal's six names by clip index (SIGNALS[i % 6], seed i // 6).  Every burst is built
once and never written.

  a      258 x 129   K = 1, 2, 3, 4 in one call; the K boundary W N = 66048 and W N + 1; clips shorter than a frame and of one sample;
                     an odd first length, so every later clip starts at an odd sample
  kbig   5 x 129     K = 65 and 71 above the 64 frames a round holds (the carry across rounds) next to K = 1, 2, 64; the largest LDS
                     need is not the first clip's
  n4096  16 x 2049   one frame per round, the one-block-per-CU LDS budget
  odd    33 x 129    partial column tile, K = 1, 2, 3
  n1024  96 x 513    N = 1024
  many   20 x 33     300 clips of 1 + (7 c mod 257) samples: starts as a running sum over many clips.  Its short tones and impulses
                     land on exact rounding ties (worst clip 1.5e-3 of its pixels), so it is held to equality with the uniform entry
                     only, never to specref.compare."""
import functools

from test_spectrogram import RATE, SIGNALS, signal

assert RATE == 24000 and len(SIGNALS) == 6
BURSTS = {
    "a": (258, 129, (66049, 100, 72000, 256, 37, 5001, 66048, 1, 200001, 257, 255, 132097)),
    "kbig": (5, 129, (81921, 1281, 90000, 37, 1280, 81920)),
    "n4096": (16, 2049, (65537, 999, 65536, 24001)),
    "odd": (33, 129, (8449, 3, 16897, 777, 8448, 12001, 5001)),
    "n1024": (96, 513, (98305, 511, 98304, 24000)),
    "many": (20, 33, tuple(1 + (7 * c) % 257 for c in range(300))),
}
COMPARED = ("a", "kbig", "n4096", "odd", "n1024")                # the bursts whose restatement stays inside specref.compare's tie cap
# the resampled burst: 48 kHz -> 24 kHz at 258 x 129
RESAMPLED = dict(width=258, height=129, rate_in=48000, rate_out=24000, lens=(48001, 3, 97, 132097, 9601))
SPEC_FMAX = 64                                                   # frames per round at most (spectrogram.hip)


def _clips(lens):
    return tuple(signal(SIGNALS[i % 6], n, seed=i // 6) for i, n in enumerate(lens))      # (read-only arrays, cached there)


@functools.lru_cache(maxsize=None)
def burst(name):
    """-> (width, height, the clips)"""
    width, height, lens = BURSTS[name]
    return width, height, _clips(lens)


@functools.lru_cache(maxsize=None)
def resampled_burst():
    return _clips(RESAMPLED["lens"])


def frames_per_column(n, width, height):
    return max(1, -(-n // (width * 2 * (height - 1))))


def workspace_bytes(n_clips):
    """bnhip.h: one 24-byte row per clip, rounded up to 256 bytes."""
    return (24 * n_clips + 255) & ~255
