"""Clip loudness normalisation: the surface of the reference's internal/audiocore/audionorm and pcmgain packages that the clip
export and the BirdWeather upload see, over bnhip_loudness_normalize_pcm16.

  Options / DefaultOptions           audionorm.go:40-75         -> Options / default_options
  PlanGain                           audionorm.go:181-202       -> plan_gain          (host arithmetic)
  ClampGainDB                        audionorm.go:217-229       -> clamp_gain_db      (host arithmetic)
  FactorFromDB                       pcmgain.go:27-32           -> factor_from_db     (host arithmetic)
  planNativeNormalizationGain        actions_database.go:1392   -> normalize_clips(.., max_gain_db=EXPORT_MAX_GAIN_DB, gate_fallback=True)
  PlanClampedGainInt16Bytes          audionorm.go:252-260       -> normalize_clips(.., max_gain_db=DEFAULT_MAX_GAIN_DB)

Mono int16 only.  The measurement follows the project's spec: the reference's float32 coefficients, evaluated in float64.
"""
import math
from dataclasses import dataclass

import numpy as np

from . import host as _host

DEFAULT_MAX_GAIN_DB = 30.0        # audionorm.DefaultMaxGainDB: the BirdWeather upload's clamp
EXPORT_MAX_GAIN_DB = 60.0         # nativeExportMaxGainDB (actions_database.go:1323): the clip export's clamp
MIN_TARGET_LUFS = -70.0           # the absolute gate: targets lie in (-70, 0)


@dataclass(frozen=True)
class Options:
    target_lufs: float = -23.0    # EBU R 128
    true_peak_dbtp: float = -1.0


def default_options():
    return Options()


@dataclass(frozen=True)
class Plan:
    target_gain_db: float
    gain_db: float
    output_lufs: float
    peak_limited: bool


def plan_gain(integrated_lufs, true_peak_dbtp, opts=None):
    """PlanGain: the gain that brings a measured clip to the target without its true peak passing the ceiling; -inf plans nothing."""
    opts = opts or default_options()
    if integrated_lufs == -math.inf:
        return Plan(0.0, 0.0, -math.inf, False)
    target_gain = opts.target_lufs - integrated_lufs
    gain, limited = target_gain, False
    if true_peak_dbtp != -math.inf:
        headroom = opts.true_peak_dbtp - true_peak_dbtp
        if gain > headroom:
            gain, limited = headroom, True
    return Plan(target_gain, gain, integrated_lufs + gain, limited)


def clamp_gain_db(gain_db, max_abs_db):
    """ClampGainDB -> (clamped, limited); max_abs_db is a magnitude."""
    lim = abs(max_abs_db)
    if gain_db > lim:
        return lim, True
    if gain_db < -lim:
        return -lim, True
    return gain_db, False


def factor_from_db(gain_db):
    """FactorFromDB: exactly 1 at 0 dB."""
    return 1.0 if gain_db == 0 else math.pow(10.0, gain_db / 20.0)


def _burst(clips):
    """The clips as contiguous arrays and their indices grouped by length (one device call per length)."""
    clips = [np.ascontiguousarray(c) for c in clips]
    for c in clips:
        if c.dtype != np.int16 or c.ndim != 1 or c.size == 0:
            raise _host.HipError(_host.E_UNSUPPORTED if c.ndim != 1 or c.dtype != np.int16 else _host.E_INVALID,
                                 "clips must be non-empty mono int16 arrays")
    groups = {}
    for i, c in enumerate(clips):
        groups.setdefault(c.size, []).append(i)
    return clips, groups


def normalize_clips(clips, sample_rate, opts=None, max_gain_db=DEFAULT_MAX_GAIN_DB, gate_fallback=False, apply=True, device=0, ragged=False):
    """A burst of detections: a list of int16 mono clips of any lengths -> (list of host.Loudness, list of int16 outputs or None),
    both in the input's order.  Clips are grouped by length, one device call per length; ragged: the whole burst in one device call
    (bnhip_loudness_ragged_normalize_pcm16) instead."""
    opts = opts or default_options()
    clips, groups = _burst(clips)
    if ragged:
        return _host.loudness_normalize_ragged(clips, sample_rate, opts.target_lufs, opts.true_peak_dbtp, max_gain_db, gate_fallback, apply,
                                               device=device)
    results, outputs = [None] * len(clips), [None] * len(clips)
    for idx in groups.values():
        res, out = _host.loudness_normalize(np.stack([clips[i] for i in idx]), sample_rate, opts.target_lufs, opts.true_peak_dbtp,
                                            max_gain_db, gate_fallback, apply, device=device)
        for j, i in enumerate(idx):
            results[i] = res[j]
            if apply:
                outputs[i] = out[j]
    return results, (outputs if apply else None)
