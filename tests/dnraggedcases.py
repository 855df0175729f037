"""The ragged denoiser's test bursts, shared by tests/test_denoise_ragged_ref.py (the tie cap of every burst and the argument errors,
CPU) and tests/test_denoise_ragged.py (the device against the restatement tests/dnref.py and against the uniform entries).

All at 24 kHz, medium preset.  Clip i of a burst is signal dncases.ABOVE_FLOOR[i % 6] at seed i // 6.  Each length is the smallest at
which a per-clip mechanism can go wrong (h = N / 4 is the hop, T the hops per block, F the frames per round):

  tiles   N = 64 (h = 16, T = 8): one sample, below a hop, exactly one hop and one over, exactly one tile (128) and one over, a
          partial last tile and hop; the odd first length puts later clips on odd offsets; shortest clips first, in the middle, last
  rounds  N = 4096: F = 2 < T + 3, so the carry across rounds runs per clip; exactly T hops (8192) and one over; the one-block-per-CU
          LDS budget
  n1024   the preset frame at 24 kHz; hop boundary +-1
  n256    another pass structure
  many    300 clips of 1 + (7 c mod 257) samples: starts and tile counts as running sums over many clips, most clips 1-2 tiles
  wide    1077 tiles at T = 64 (>= 1024), so the plan keeps T = 64 where the uniform call of the third clip alone picks T = 8: bytes
          must not depend on T

A burst's seed is changed, never the cap, if its signals trip the tie cap (dnref.check_cap, over the clips of a burst together)."""
import functools

import numpy as np

import dncases
import dnref

RATE = dncases.RATE
NR_DB, NF_DB = (float(v) for v in dnref.PRESETS["medium"])

# name -> (N, lens)
BURSTS = {
    "tiles": (64, (4999, 1, 7, 16, 17, 128, 129, 37, 127, 2063, 112, 113)),
    "rounds": (4096, (40963, 999, 4096, 8192, 8193, 1)),
    "n1024": (1024, (5197, 255, 256, 257, 24000, 2048, 2049)),
    "n256": (256, (4099, 63, 64, 65, 1024, 511, 513)),
    "many": (64, tuple(1 + (7 * c) % 257 for c in range(300))),
    "wide": (64, (600001, 500003, 1025)),
}
# the chain's burst: the loudness sub-block at 24 kHz is S = 2400 samples - none, below one, exactly one, one over, ten, five and a bit
CHAIN_LENS = (1, 2399, 2400, 2401, 24000, 37, 12001)


def burst_clips(lens):
    """The list of int16 clips of these lengths, read-only."""
    return [dncases.signal(dncases.ABOVE_FLOOR[i % 6], int(n), i // 6) for i, n in enumerate(lens)]


def frame(name):
    return BURSTS[name][0]


def clips(name):
    return burst_clips(BURSTS[name][1])


@functools.lru_cache(maxsize=None)
def restated(name):
    """(int16 [total], v float64 [total]) of a burst, the clips one after another: computed once, shared, read-only."""
    N = frame(name)
    v = np.concatenate([dnref.denoise(c, N, NR_DB, NF_DB) for c in clips(name)])
    q = dnref.quant(v)
    q.setflags(write=False)
    v.setflags(write=False)
    return q, v


def workspace_formula(n_clips):
    """What bnhip.h documents: two tables of n_clips + 1 64-bit entries, rounded up to 256 bytes."""
    return (2 * (n_clips + 1) * 8 + 255) // 256 * 256
