"""Processed audio: the review UI's denoise / normalise / gain of a saved clip, over bnhip_denoise_pcm16 and bnhip_process_pcm16, their
ragged forms for a burst of clips of unequal lengths, and the chain fused with the spectrogram render and its PNG encoder
(bnhip_process_spectrogram_png_ragged_pcm16).

  denoisePresets / IsValidDenoisePreset   ffmpeg/process.go:181-195     -> DENOISE_PRESETS / is_valid_denoise_preset
  MaxGainDB / IsValidGainDB               ffmpeg/process.go:197-203     -> MAX_GAIN_DB / is_valid_gain_db
  BuildProcessingFilterChain              ffmpeg/process.go:212-251     -> process_clips   (denoise -> normalise -> gain)
  ProcessAudioByID                        api/v2/media/media.go:1200    -> process_clips
  ProcessedSpectrogramByID                api/v2/media/media.go:1321    -> processed_spectrogram

Mono int16 clips: a batch of one length, or with ragged=True / fused=True a list of any lengths.  The denoiser follows the project's spec (DESIGN.md §9 "Denoise"), not FFmpeg's afftdn: FFmpeg is not
in the reference's tree.  Each stage hands int16 to the next, where FFmpeg's chain stays in float until its output.
"""
import math
import os

import numpy as np

from . import host as _host
from . import spectrogram as _spectrogram

DENOISE_PRESETS = {"light": (6, -30), "medium": (12, -40), "heavy": (20, -50)}      # name -> (nr_db, nf_db)
MAX_GAIN_DB = 60.0
LOUDNORM_TARGET_I, LOUDNORM_TARGET_TP = -23.0, -2.0                                  # loudnormTargetI / TP (process.go:205-210)
FRAME_SECONDS = 0.04                                                                 # the frame's nominal length
FRAME_MIN, FRAME_MAX = 64, 4096


def is_valid_denoise_preset(preset):
    """IsValidDenoisePreset: a preset's name, or "" for off."""
    return preset == "" or preset in DENOISE_PRESETS


def is_valid_gain_db(gain_db):
    """IsValidGainDB: finite and within +-MAX_GAIN_DB."""
    return isinstance(gain_db, (int, float)) and math.isfinite(gain_db) and -MAX_GAIN_DB <= gain_db <= MAX_GAIN_DB


def frame_for_rate(rate):
    """The frame length for clips at `rate` Hz: the power of two nearest (in log2) to 40 ms, within 64..4096."""
    if rate <= 0:
        raise ValueError("sample rate must be positive")
    return int(min(FRAME_MAX, max(FRAME_MIN, 2 ** int(math.floor(math.log2(FRAME_SECONDS * rate) + 0.5)))))


def _denoise_params(sample_rate, preset, nr_db=None, nf_db=None, frame=None):
    if not is_valid_denoise_preset(preset) or preset == "" and (nr_db is None or nf_db is None):
        raise ValueError(f'invalid denoise preset "{preset}" (valid: light, medium, heavy)')
    p_nr, p_nf = DENOISE_PRESETS.get(preset, (None, None))
    return (frame_for_rate(sample_rate) if frame is None else int(frame), float(p_nr if nr_db is None else nr_db),
            float(p_nf if nf_db is None else nf_db))


def _ragged_list(clips):
    """A burst as a list of 1-D clips: a list as it is, an [n_clips, n] array row by row."""
    return list(clips) if isinstance(clips, (list, tuple)) else list(np.atleast_2d(np.asarray(clips)))


def denoise_clips(clips, sample_rate, preset="medium", nr_db=None, nf_db=None, frame=None, device=0, ragged=False):
    """int16 [n_clips, n] (or [n]) -> the denoised int16 [n_clips, n] in one device call.  preset names (nr_db, nf_db); either may
    be given instead; frame defaults to frame_for_rate(sample_rate).  ragged: a list of 1-D int16 clips of any lengths -> the list of
    denoised clips, still one call (bnhip_denoise_ragged_pcm16)."""
    frame, nr_db, nf_db = _denoise_params(sample_rate, preset, nr_db, nf_db, frame)
    if ragged:
        return _host.denoise_ragged(_ragged_list(clips), frame, nr_db, nf_db, device=device)
    return _host.denoise(clips, frame, nr_db, nf_db, device=device)


def _chain_params(sample_rate, denoise, normalize, gain_db):
    if not is_valid_denoise_preset(denoise):
        raise ValueError(f'invalid denoise preset "{denoise}" (valid: "", light, medium, heavy)')
    if not is_valid_gain_db(gain_db):
        raise ValueError("gain_db must be between -60 and 60 dB")
    if denoise == "" and not normalize and gain_db == 0:
        raise ValueError("no filter active: one of denoise, normalize, gain_db is required")
    return _denoise_params(sample_rate, denoise) if denoise else (0, 0.0, -40.0)


def process_clips(clips, sample_rate, denoise="", normalize=False, gain_db=0.0, device=0, ragged=False):
    """The chain of ProcessAudioByID on a batch: int16 [n_clips, n] -> (int16 [n_clips, n], list of host.Loudness or None without
    normalize), one call of bnhip_process_pcm16, the clips staying on the device between the stages.  Normalisation aims at the
    reference's loudnorm targets (-23 LUFS, -2 dBTP).  ragged: a list of 1-D int16 clips of any lengths -> (list of clips, records),
    one call of bnhip_process_ragged_pcm16."""
    frame, nr_db, nf_db = _chain_params(sample_rate, denoise, normalize, gain_db)
    if ragged:
        return _host.process_ragged(_ragged_list(clips), sample_rate, frame, nr_db, nf_db, normalize, LOUDNORM_TARGET_I, LOUDNORM_TARGET_TP,
                                    gain_db, device=device)
    return _host.process(clips, sample_rate, frame, nr_db, nf_db, normalize, LOUDNORM_TARGET_I, LOUDNORM_TARGET_TP, gain_db, device=device)


def processed_spectrogram(clips, output_paths, width, sample_rate, denoise="", normalize=False, gain_db=0.0, device=0, fused=False,
                          **spectrogram_kwargs):
    """ProcessedSpectrogramByID on a batch: the chain, then one PNG per processed clip at output_paths[i] -> the uint8 [B, H, W]
    indices.  Two device calls (process_clips, then spectrogram.generate_batch with device_png), the processed PCM passing through
    the host between them.  With no filter active it raises: the reference serves the unprocessed spectrogram for such a request
    (media.go:1338-1341), which here is spectrogram.generate_batch itself.  fused: one device call
    (bnhip_process_spectrogram_png_ragged_pcm16), the processed PCM staying on the device; clips may then also be a list of 1-D
    int16 clips of any lengths.  The files and the indices are those of the two calls."""
    if not fused:
        pcm, _ = process_clips(clips, sample_rate, denoise, normalize, gain_db, device=device)
        return _spectrogram.generate_batch(pcm, output_paths, width, sample_rate, device=device, device_png=True, **spectrogram_kwargs)
    frame, nr_db, nf_db = _chain_params(sample_rate, denoise, normalize, gain_db)
    burst = _ragged_list(clips)
    if not burst or len(burst) != len(output_paths):
        raise ValueError("a burst is a non-empty sequence of clips with one output path per clip")
    for p in output_paths:
        if not p or not os.path.isabs(p):
            raise ValueError("output path must be absolute")
    style = spectrogram_kwargs.get("style", "default")
    kw = _spectrogram._render_args(sample_rate, width, spectrogram_kwargs.get("profile"), style, spectrogram_kwargs.get("dynamic_range", "100"))
    extra = set(spectrogram_kwargs) - {"profile", "style", "dynamic_range"}
    if extra:
        raise TypeError(f"unexpected keyword arguments: {sorted(extra)}")
    streams, _, _ = _host.process_spectrogram_png_ragged(burst, sample_rate, width, _spectrogram.palette(style), frame, nr_db, nf_db, normalize,
                                                         LOUDNORM_TARGET_I, LOUDNORM_TARGET_TP, gain_db, device=device, **kw)
    for p, s in zip(output_paths, streams):
        with open(p, "wb") as fh:
            fh.write(s)
    return np.stack([_spectrogram.read_png_indices(s) for s in streams])
