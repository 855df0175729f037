"""Host-side mirror of the reference's backend interface over the C ABI (ctypes).

Mirrors, name for name, the Go seam this engine drops in behind:
  inference.Classifier          internal/inference/backend.go:8-19   -> HipClassifier.predict/num_species/close
  inference.EmbeddingExtractor  internal/inference/backend.go:21-29  -> HipClassifier.predict_with_embeddings
  onnx.Classifier.PredictBatch  internal/inference/onnx/classifier.go:372-430 -> HipClassifier.predict_batch
  (*BirdNET).Predict post-proc  internal/classifier/analyze.go:25-110 -> BirdNET.predict (sigmoid(sens) + top-10)
Error behaviour follows the reference: size mismatch is an error (tflite/classifier.go:102-104), the
"backend unavailable" condition is a distinct sentinel so callers can fall back
(openvino/openvino.go:26-31 ErrOpenVINOUnavailable), and nothing ever silently falls back to a CPU path.

This file is plumbing for tests/bench in this repo (Go is not installed here); the production
binding is the cgo file under go/ (see INTEGRATION.md).
"""
import collections
import ctypes as C
import json
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
TUNE_DIR = os.path.join(_HERE, "tune")             # recorded create-time tunings shipped with the package (bnhip.h "tune_dir")
LIB_PATH = os.environ.get("BNHIP_LIB") or os.path.join(_HERE, "lib", "libbnhip.so")   # BNHIP_LIB: A/B a second build

BNHIP_OK, E_INVALID, E_NO_DEVICE, E_MODEL, E_UNSUPPORTED, E_RUNTIME, E_NOMEM = 0, -1, -2, -3, -4, -5, -6

SYMBOLS = ["bnhip_init", "bnhip_shutdown", "bnhip_model_create", "bnhip_model_info", "bnhip_predict",
           "bnhip_predict_pcm16", "bnhip_predict_pcm", "bnhip_predict_device", "bnhip_postprocess_topk", "bnhip_predict_topk",
           "bnhip_us_frame_cv", "bnhip_set_stream", "bnhip_synchronize", "bnhip_profile_enable",
           "bnhip_profile_read", "bnhip_model_describe", "bnhip_model_destroy", "bnhip_last_error",
           "bnhip_version", "bnhip_debug_fetch", "bnhip_profile_filter", "bnhip_resample_length",
           "bnhip_resample_f32", "bnhip_resample_pcm16", "bnhip_model_devices", "bnhip_last_error_copy",
           "bnhip_resampler_create", "bnhip_resampler_estimate", "bnhip_resampler_process_pcm16",
           "bnhip_resampler_process_f32", "bnhip_resampler_flush_pcm16", "bnhip_resampler_flush_f32",
           "bnhip_resampler_destroy", "bnhip_us_frame_cv_device", "bnhip_profile_steps", "bnhip_profile_steps_read",
           "bnhip_host_alloc", "bnhip_host_free", "bnhip_windows_create", "bnhip_windows_info", "bnhip_windows_add_source",
           "bnhip_windows_remove_source", "bnhip_windows_write", "bnhip_windows_collect", "bnhip_windows_ready",
           "bnhip_windows_stats", "bnhip_windows_reset", "bnhip_windows_destroy", "bnhip_predict_pcm_topk",
           "bnhip_windows_predict_topk", "bnhip_resampler_bank_create", "bnhip_resampler_bank_add_stream",
           "bnhip_resampler_bank_remove_stream", "bnhip_resampler_bank_estimate", "bnhip_resampler_bank_process_pcm16",
           "bnhip_resampler_bank_flush_pcm16", "bnhip_windows_write_resampled", "bnhip_resampler_bank_destroy",
           "bnhip_eq_bank_create", "bnhip_eq_bank_add_stream", "bnhip_eq_bank_remove_stream", "bnhip_eq_bank_set_chain",
           "bnhip_eq_bank_reset", "bnhip_eq_bank_process_pcm16", "bnhip_windows_write_equalized", "bnhip_eq_design",
           "bnhip_eq_bank_destroy", "bnhip_soundlevel_bands", "bnhip_soundlevel_bank_create", "bnhip_soundlevel_bank_add_stream",
           "bnhip_soundlevel_bank_remove_stream", "bnhip_soundlevel_bank_reset", "bnhip_soundlevel_bank_process_pcm16",
           "bnhip_soundlevel_bank_destroy", "bnhip_range_heatmap", "bnhip_spectrogram_size", "bnhip_spectrogram_pcm16",
           "bnhip_spectrogram_device", "bnhip_loudness_measure_pcm16", "bnhip_loudness_normalize_pcm16",
           "bnhip_loudness_workspace_size", "bnhip_loudness_normalize_device", "bnhip_flac_max_bytes", "bnhip_flac_workspace_size",
           "bnhip_flac_encode_device", "bnhip_flac_encode_pcm16", "bnhip_loudness_flac_pcm16", "bnhip_flac_lpc_workspace_size",
           "bnhip_flac_lpc_encode_device", "bnhip_flac_lpc_encode_pcm16", "bnhip_loudness_flac_lpc_pcm16",
           "bnhip_loudness_ragged_workspace_size", "bnhip_loudness_ragged_normalize_pcm16", "bnhip_loudness_ragged_normalize_device",
           "bnhip_flac_ragged_max_bytes", "bnhip_flac_ragged_workspace_size", "bnhip_flac_ragged_encode_device",
           "bnhip_flac_ragged_encode_pcm16", "bnhip_loudness_flac_ragged_pcm16", "bnhip_png_max_bytes", "bnhip_png_workspace_size",
           "bnhip_png_encode_device", "bnhip_png_encode_u8", "bnhip_spectrogram_png_pcm16", "bnhip_spectrogram_ragged_workspace_size",
           "bnhip_spectrogram_ragged_pcm16", "bnhip_spectrogram_png_ragged_pcm16", "bnhip_spectrogram_ragged_device",
           "bnhip_flac_stream_info", "bnhip_flac_decode_workspace_size", "bnhip_flac_decode_device", "bnhip_flac_decode_pcm16",
           "bnhip_flac_spectrogram_png", "bnhip_denoise_workspace_size", "bnhip_denoise_device", "bnhip_denoise_pcm16",
           "bnhip_process_pcm16", "bnhip_denoise_ragged_workspace_size", "bnhip_denoise_ragged_device", "bnhip_denoise_ragged_pcm16",
           "bnhip_process_ragged_pcm16", "bnhip_process_spectrogram_png_ragged_pcm16", "bnhip_analyze_windows",
           "bnhip_analyze_pcm_topk", "bnhip_analyze_pcm", "bnhip_analyze_mixed_windows", "bnhip_analyze_mixed_pcm_topk",
           "bnhip_analyze_mixed_pcm", "bnhip_analyze_channels_windows", "bnhip_analyze_channels_pcm_topk",
           "bnhip_analyze_channels_pcm", "bnhip_channel_energy_pcm", "bnhip_analyze_pcm_events", "bnhip_analyze_mixed_pcm_events",
           "bnhip_analyze_channels_pcm_events", "bnhip_detection_events", "bnhip_event_min_count",
           "bnhip_event_clip_spans", "bnhip_recording_clips_pcm16", "bnhip_analyze_channels_pcm_clips", "bnhip_event_bank_create",
           "bnhip_event_bank_info", "bnhip_event_bank_set_filter", "bnhip_event_bank_process", "bnhip_event_bank_process_device",
           "bnhip_event_bank_flush", "bnhip_event_bank_reset", "bnhip_event_bank_pending", "bnhip_event_bank_clock",
           "bnhip_event_bank_destroy", "bnhip_windows_predict_events", "bnhip_capture_bank_create", "bnhip_capture_bank_info",
           "bnhip_capture_bank_positions", "bnhip_capture_bank_reset", "bnhip_capture_bank_write", "bnhip_capture_bank_read_pcm16",
           "bnhip_capture_bank_clips", "bnhip_capture_bank_destroy", "bnhip_capture_spans", "bnhip_detection_events_extended",
           "bnhip_analyze_channels_pcm_events_extended", "bnhip_analyze_channels_pcm_clips_extended",
           "bnhip_event_bank_create_extended", "bnhip_event_bank_set_extend", "bnhip_event_deadline",
           "bnhip_event_bank_create_dynamic", "bnhip_event_bank_set_dynamic", "bnhip_event_bank_set_now",
           "bnhip_event_bank_threshold_changes", "bnhip_event_bank_thresholds", "bnhip_event_bank_set_thresholds",
           "bnhip_event_bank_reset_thresholds", "bnhip_event_threshold", "bnhip_audio_level", "bnhip_level_bank_create",
           "bnhip_level_bank_add_stream", "bnhip_level_bank_remove_stream", "bnhip_level_bank_process_pcm", "bnhip_level_bank_latest",
           "bnhip_level_bank_stats", "bnhip_level_bank_reset", "bnhip_level_bank_destroy", "bnhip_capture_bank_write_levels",
           "bnhip_detection_events_guarded", "bnhip_analyze_channels_pcm_events_guarded", "bnhip_analyze_channels_pcm_clips_guarded",
           "bnhip_event_bank_set_guards", "bnhip_event_bank_set_daylight", "bnhip_flac_recording_info",
           "bnhip_flac_decode_recordings_workspace_size", "bnhip_flac_decode_recordings_device", "bnhip_flac_decode_recordings",
           "bnhip_analyze_flac_windows", "bnhip_analyze_flac_topk", "bnhip_analyze_flac", "bnhip_analyze_flac_events"]


class HipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"bnhip error {code}: {msg}")
        self.code = code


class ErrHIPUnavailable(HipError):
    """Sentinel like openvino.ErrOpenVINOUnavailable: library missing / no gfx950 device."""


_lib = None


def load_library(path=None):
    """Loads libbnhip.so; fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ErrHIPUnavailable(E_NO_DEVICE, f"{p} not built (run `python -c 'import __graft_entry__ as g; g.build()'`)")
    lib = C.CDLL(p)
    lib.bnhip_last_error.restype = C.c_char_p
    lib.bnhip_version.restype = C.c_char_p
    lib.bnhip_model_create.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.POINTER(C.c_void_p)]
    lib.bnhip_model_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.bnhip_predict.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.bnhip_predict_pcm16.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.bnhip_predict_pcm.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.bnhip_predict_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.bnhip_postprocess_topk.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int,
                                           C.c_void_p, C.c_void_p]
    lib.bnhip_predict_topk.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p,
                                       C.c_void_p]
    lib.bnhip_predict_pcm_topk.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p,
                                           C.c_void_p]
    lib.bnhip_us_frame_cv.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p]
    lib.bnhip_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.bnhip_synchronize.argtypes = [C.c_void_p]
    lib.bnhip_profile_enable.argtypes = [C.c_void_p, C.c_int]
    lib.bnhip_profile_read.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    lib.bnhip_profile_filter.argtypes = [C.c_void_p, C.c_char_p]
    lib.bnhip_model_describe.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    lib.bnhip_model_destroy.argtypes = [C.c_void_p]
    lib.bnhip_init.argtypes = [C.POINTER(C.c_int)]
    if path is None:
        _lib = lib
    return lib


def _check(lib, rc):
    if rc != BNHIP_OK:
        msg = (lib.bnhip_last_error() or b"").decode("utf-8", "replace")
        raise (ErrHIPUnavailable if rc == E_NO_DEVICE else HipError)(rc, msg)


def _analyze_protos(lib):
    """ctypes prototypes of the file-analysis entries (set at use, as for the other later entries: load_library must go on
    loading a library that predates them)."""
    lib.bnhip_analyze_windows.restype = C.c_longlong
    lib.bnhip_analyze_windows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p]
    lib.bnhip_analyze_pcm_topk.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_double,
                                           C.c_int, C.c_void_p, C.c_void_p]
    lib.bnhip_analyze_pcm.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_double,
                                      C.c_int, C.c_float, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    return lib


def _analyze_mixed_protos(lib):
    """... and of the entries for recordings at their own rates and depths (apart, so that the entries above go on working on a
    library that predates these)."""
    _analyze_protos(lib)
    lib.bnhip_analyze_mixed_windows.restype = C.c_longlong
    lib.bnhip_analyze_mixed_windows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
    lib.bnhip_analyze_mixed_pcm_topk.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_double,
                                                 C.c_int, C.c_void_p, C.c_void_p]
    lib.bnhip_analyze_mixed_pcm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_double,
                                            C.c_int, C.c_float, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    return lib


# one row of bnhip_analyze_pcm (bnhip_detection)
DETECTION = np.dtype([("recording", "<i4"), ("window", "<i4"), ("class_index", "<i4"), ("confidence", "<f4")])
# one recording of the mixed entries (bnhip_recording): samples at its own rate, the rate, the depth (0 = float32)
RECORDING = np.dtype([("length", "<i8"), ("rate", "<i4"), ("bits_per_sample", "<i4")])


def recordings(lengths, rates, depths):
    """-> the RECORDING table of recordings of `lengths` samples at `rates` Hz and `depths` bits (scalars are broadcast)."""
    ln = np.asarray(lengths, np.int64).reshape(-1)
    recs = np.zeros(ln.size, RECORDING)
    recs["length"], recs["rate"], recs["bits_per_sample"] = ln, rates, depths
    return recs


def _analyze_channels_protos(lib):
    """... and of the entries for multichannel recordings (apart again, for the same reason)."""
    _analyze_mixed_protos(lib)
    lib.bnhip_analyze_channels_windows.restype = C.c_longlong
    lib.bnhip_analyze_channels_windows.argtypes = lib.bnhip_analyze_mixed_windows.argtypes
    lib.bnhip_analyze_channels_pcm_topk.argtypes = lib.bnhip_analyze_mixed_pcm_topk.argtypes + [C.c_void_p]
    lib.bnhip_analyze_channels_pcm.argtypes = lib.bnhip_analyze_mixed_pcm.argtypes + [C.c_void_p]
    lib.bnhip_channel_energy_pcm.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return lib


# one recording of the channels entries (bnhip_channels_recording): frames at its own rate, the rate, the depth, the channels of a
# frame and which of them is read (a channel index, CHANNEL_MIX or CHANNEL_AUTO)
CHANNELS_RECORDING = np.dtype([("length", "<i8"), ("rate", "<i4"), ("bits_per_sample", "<i4"), ("channels", "<i4"), ("select", "<i4")])
# one channel of bnhip_channel_energy_pcm (bnhip_channel_energy): the exact sum of squares in 128 bits, and its level
CHANNEL_ENERGY = np.dtype([("sum_lo", "<u8"), ("sum_hi", "<u8"), ("rms_dbfs", "<f8")])
CHANNEL_MIX, CHANNEL_AUTO = -1, -2


def channel_select(choice):
    """A channel index, "mix" or "auto" -> the `select` of a CHANNELS_RECORDING."""
    return {"mix": CHANNEL_MIX, "auto": CHANNEL_AUTO}[choice] if isinstance(choice, str) else int(choice)


def channel_recordings(lengths, rates, depths, channels, select=0):
    """-> the CHANNELS_RECORDING table of recordings of `lengths` frames of `channels` interleaved samples at `rates` Hz and `depths`
    bits; select: per recording (or one for all) a channel index, "mix" / CHANNEL_MIX or "auto" / CHANNEL_AUTO."""
    ln = np.asarray(lengths, np.int64).reshape(-1)
    recs = np.zeros(ln.size, CHANNELS_RECORDING)
    recs["length"], recs["rate"], recs["bits_per_sample"], recs["channels"] = ln, rates, depths, channels
    recs["select"] = [channel_select(s) for s in select] if isinstance(select, (list, tuple)) else channel_select(select)
    return recs


def _checked_bytes(raw, depths, samples, expected):
    """The bytes of a file-analysis call as a uint8 array, checked against the depth(s) and sample count(s) of its recordings."""
    x = np.frombuffer(raw, np.uint8) if not isinstance(raw, np.ndarray) else np.ascontiguousarray(raw).reshape(-1).view(np.uint8)
    depths, samples = np.atleast_1d(depths), np.atleast_1d(samples)
    bad = ~np.isin(depths, (0, 16, 24, 32))
    if bad.any():
        raise HipError(E_INVALID, f"unsupported bit depth: {int(depths[bad][0])} (supported: 0 = float32, 16, 24, 32)")
    bps = np.where(depths == 0, 4, depths // 8)
    want = int((samples * bps).sum())
    if x.size != want:
        raise HipError(E_INVALID, "input size mismatch: " + expected.format(want=want, samples=int(samples.sum()), bps=int(bps[0]) if bps.size else 0) + f", got {x.size} bytes")
    return x


def _channels_bytes(raw, recs):
    """The interleaved bytes of a channels call as a uint8 array, checked against the table."""
    recs = np.ascontiguousarray(recs, CHANNELS_RECORDING).reshape(-1)
    return _checked_bytes(raw, recs["bits_per_sample"], recs["length"] * recs["channels"].astype(np.int64), "the recordings hold {want} bytes"), recs


def _analyze_events_protos(lib):
    """... and of the detection-event entries (apart again, for the same reason)."""
    _analyze_channels_protos(lib)
    tail = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]                # filter, out, cap, n_out
    lib.bnhip_analyze_pcm_events.argtypes = lib.bnhip_analyze_pcm.argtypes[:10] + tail
    lib.bnhip_analyze_mixed_pcm_events.argtypes = lib.bnhip_analyze_mixed_pcm.argtypes[:10] + tail
    lib.bnhip_analyze_channels_pcm_events.argtypes = lib.bnhip_analyze_mixed_pcm.argtypes[:10] + tail + [C.c_void_p]
    lib.bnhip_detection_events.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int] + tail
    lib.bnhip_event_min_count.argtypes = [C.c_int, C.c_double]
    xtail = [C.c_void_p] + tail                                                       # filter, extend, out, cap, n_out
    lib.bnhip_analyze_channels_pcm_events_extended.argtypes = lib.bnhip_analyze_mixed_pcm.argtypes[:10] + xtail + [C.c_void_p]
    lib.bnhip_detection_events_extended.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int] + xtail
    gtail = [C.c_void_p] + xtail                                                      # filter, extend, guards, out, cap, n_out
    lib.bnhip_analyze_channels_pcm_events_guarded.argtypes = lib.bnhip_analyze_mixed_pcm.argtypes[:10] + gtail + [C.c_void_p]
    lib.bnhip_detection_events_guarded.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_int] + gtail
    lib.bnhip_event_deadline.argtypes = [C.c_int32, C.c_void_p, C.c_int64, C.c_int64]
    lib.bnhip_event_deadline.restype = C.c_int64
    return lib


# one event of the *_events entries (bnhip_event)
EVENT = np.dtype([("recording", "<i4"), ("class_index", "<i4"), ("first_window", "<i4"), ("last_window", "<i4"), ("best_window", "<i4"),
                  ("count", "<i4"), ("confidence", "<f4"), ("status", "<i4")])
EVENTS_KEEP_DROPPED = 1
EVENT_KEPT, EVENT_FEW, EVENT_VETOED, EVENT_DOG, EVENT_DAYLIGHT = 0, 1, 2, 3, 4
EVENT_DAYLIGHT_SPANS = 8


class _EventFilterStruct(C.Structure):
    _fields_ = [("class_threshold", C.c_void_p), ("class_veto", C.c_void_p), ("veto_threshold", C.c_float), ("hold_windows", C.c_int32),
                ("min_count", C.c_int32), ("flags", C.c_int32)]


class EventTables:
    """The filter of the *_events entries (bnhip_event_filter) as its tables: class_threshold float32 [n_classes] (a hit is
    confidence > class_threshold[class]: +inf or NaN excludes the class), class_veto uint8 [n_classes] or None, veto_threshold,
    hold_windows, min_count, flags (EVENTS_KEEP_DROPPED).  wav.EventFilter builds one from lists and seconds."""

    def __init__(self, class_threshold, class_veto=None, veto_threshold=0.0, hold_windows=1, min_count=1, flags=0):
        self.class_threshold = np.ascontiguousarray(class_threshold, np.float32).reshape(-1)
        self.class_veto = None if class_veto is None else np.ascontiguousarray(class_veto, np.uint8).reshape(-1)
        self.veto_threshold, self.hold_windows, self.min_count, self.flags = float(veto_threshold), int(hold_windows), int(min_count), int(flags)

    def _struct(self, n_classes):
        """-> the C struct; the tables must hold n_classes entries each (the arrays stay alive with self)."""
        if self.class_threshold.size != n_classes or (self.class_veto is not None and self.class_veto.size != n_classes):
            raise HipError(E_INVALID, f"the event filter's tables must hold n_classes = {n_classes} entries")
        return _EventFilterStruct(self.class_threshold.ctypes.data, None if self.class_veto is None else self.class_veto.ctypes.data,
                                  self.veto_threshold, self.hold_windows, self.min_count, self.flags)


class _EventExtendStruct(C.Structure):
    _fields_ = [("class_extended", C.c_void_p), ("max_windows", C.c_int32), ("short_wait", C.c_int32), ("medium_from", C.c_int32),
                ("medium_wait", C.c_int32), ("long_from", C.c_int32), ("long_wait", C.c_int32)]


class EventExtend:
    """Extended capture beside an EventTables (bnhip_event_extend; include/bnhip.h, "Detection events: extended capture"), in
    windows: class_extended uint8 [n_classes] (non-zero: every hit of the class moves its event's deadline) or None for every
    class, max_windows (an event opened at b is due at b + max_windows at the latest), short_wait, medium_from, medium_wait,
    long_from, long_wait.  wav.ExtendedCapture builds one from species and seconds."""

    def __init__(self, class_extended, max_windows, short_wait, medium_from, medium_wait, long_from, long_wait):
        self.class_extended = None if class_extended is None else np.ascontiguousarray(class_extended, np.uint8).reshape(-1)
        self.max_windows, self.short_wait, self.medium_from = int(max_windows), int(short_wait), int(medium_from)
        self.medium_wait, self.long_from, self.long_wait = int(medium_wait), int(long_from), int(long_wait)

    def longest_wait(self, hold_windows):
        """W: no deadline lies further behind the hit that set it."""
        return max(int(hold_windows), self.short_wait, self.medium_wait, self.long_wait)

    def _struct(self, n_classes):
        """-> the C struct; the table must hold n_classes entries (the array stays alive with self)."""
        if self.class_extended is not None and self.class_extended.size != n_classes:
            raise HipError(E_INVALID, f"the event extend's table must hold n_classes = {n_classes} entries")
        return _EventExtendStruct(None if self.class_extended is None else self.class_extended.ctypes.data, self.max_windows, self.short_wait,
                                  self.medium_from, self.medium_wait, self.long_from, self.long_wait)


class _EventGuardsStruct(C.Structure):
    _fields_ = [("class_dog", C.c_void_p), ("class_dog_filtered", C.c_void_p), ("class_daylight", C.c_void_p), ("daylight_spans", C.c_void_p),
                ("dog_threshold", C.c_float), ("dog_remember_windows", C.c_int32), ("n_spans", C.c_int32), ("reserved", C.c_int32)]


class EventGuards:
    """The dog-bark and daylight filters beside an EventTables (bnhip_event_guards; include/bnhip.h, "Detection events: dog-bark
    and daylight filters"), in windows: class_dog uint8 [n_classes] (non-zero: a result of the class above dog_threshold marks its
    window as a dog hit) or None, class_dog_filtered uint8 [n_classes] (non-zero: an event of the class is dropped with status
    EVENT_DOG when the last dog hit lies at most dog_remember_windows before its deadline) or None, class_daylight uint8 [n_classes]
    (non-zero: an event of the class that begins inside a daylight span is dropped with status EVENT_DAYLIGHT) or None, and for the
    file tail daylight_spans int32 [n_spans, 3] = (recording, from, to), ascending and disjoint, or None; a bank takes its sources'
    spans through EventBank.set_daylight and does not read these.  wav.EventGuards builds one from labels, minutes and seconds."""

    def __init__(self, class_dog=None, dog_threshold=0.0, class_dog_filtered=None, dog_remember_windows=0, class_daylight=None,
                 daylight_spans=None):
        tab = lambda t: None if t is None else np.ascontiguousarray(t, np.uint8).reshape(-1)
        self.class_dog, self.class_dog_filtered, self.class_daylight = tab(class_dog), tab(class_dog_filtered), tab(class_daylight)
        self.dog_threshold, self.dog_remember_windows = float(dog_threshold), int(dog_remember_windows)
        self.daylight_spans = None if daylight_spans is None else np.ascontiguousarray(daylight_spans, np.int32).reshape(-1, 3)

    def _struct(self, n_classes):
        """-> the C struct; the tables must hold n_classes entries each (the arrays stay alive with self)."""
        for t in (self.class_dog, self.class_dog_filtered, self.class_daylight):
            if t is not None and t.size != n_classes:
                raise HipError(E_INVALID, f"the event guards' tables must hold n_classes = {n_classes} entries")
        p = lambda t: None if t is None or t.size == 0 else t.ctypes.data
        n_spans = 0 if self.daylight_spans is None else self.daylight_spans.shape[0]
        return _EventGuardsStruct(p(self.class_dog), p(self.class_dog_filtered), p(self.class_daylight), p(self.daylight_spans),
                                  self.dog_threshold, self.dog_remember_windows, n_spans, 0)


class _EventDynamicStruct(C.Structure):
    _fields_ = [("class_dynamic", C.c_void_p), ("trigger", C.c_float), ("min_threshold", C.c_float), ("valid", C.c_int64),
                ("cooldown", C.c_int64)]


# one record of EventBank.threshold_changes (bnhip_threshold_change)
THRESHOLD_CHANGE = np.dtype([("class_index", "<i4"), ("previous_level", "<i4"), ("new_level", "<i4"), ("reason", "<i4"),
                             ("previous_value", "<f4"), ("new_value", "<f4"), ("confidence", "<f4"), ("pad", "<i4")])
THRESHOLD_EXPIRY, THRESHOLD_HIGH_CONFIDENCE = 0, 1


class EventDynamic:
    """Dynamic thresholds beside an EventTables (bnhip_event_dynamic; include/bnhip.h, "Detection events: dynamic thresholds"):
    class_dynamic uint8 [n_classes] (non-zero: the class learns; zero: a species with a custom threshold) or None for every class,
    trigger, min_threshold, and valid and cooldown in bank time (the unit of EventBank.set_now)."""

    def __init__(self, class_dynamic, trigger, min_threshold, valid, cooldown):
        self.class_dynamic = None if class_dynamic is None else np.ascontiguousarray(class_dynamic, np.uint8).reshape(-1)
        self.trigger, self.min_threshold, self.valid, self.cooldown = float(trigger), float(min_threshold), int(valid), int(cooldown)

    def _struct(self, n_classes):
        """-> the C struct; the table must hold n_classes entries (the array stays alive with self)."""
        if self.class_dynamic is not None and self.class_dynamic.size != n_classes:
            raise HipError(E_INVALID, f"the event dynamic's table must hold n_classes = {n_classes} entries")
        return _EventDynamicStruct(None if self.class_dynamic is None else self.class_dynamic.ctypes.data, self.trigger, self.min_threshold,
                                   self.valid, self.cooldown)


def event_threshold(base, level, min_threshold):
    """bnhip_event_threshold (host only): the effective threshold of a base at a level (float32)."""
    lib = _event_bank_protos(load_library())
    return np.float32(lib.bnhip_event_threshold(float(np.float32(base)), int(level), float(np.float32(min_threshold))))


def event_deadline(hold_windows, extend, first_window, window):
    """bnhip_event_deadline (host only): the deadline of an event of a sliding class opened at first_window, last hit at window."""
    lib = _analyze_events_protos(load_library())
    xs = extend._struct(extend.class_extended.size if extend.class_extended is not None else 0)
    d = lib.bnhip_event_deadline(int(hold_windows), C.addressof(xs), int(first_window), int(window))
    if d < 0:
        _check(lib, int(d))
    return int(d)


def event_min_count(level, overlap_seconds):
    """bnhip_event_min_count (host only): the reference's minimum hit count of a detection for a false-positive filter level
    (0-5) at an analysis overlap in seconds."""
    return int(_analyze_events_protos(load_library()).bnhip_event_min_count(int(level), float(overlap_seconds)))


def detection_events(rows, n_classes, filter, device=0, cap=None, extend=None, guards=None):
    """bnhip_detection_events: the event tail alone over DETECTION rows the host holds (nondecreasing in (recording, window));
    with extend (an EventExtend) bnhip_detection_events_extended; with guards (an EventGuards) bnhip_detection_events_guarded,
    under the extend or none.
    -> the events (EVENT), ascending by (recording, class_index, first_window); with cap -> (events[:cap], total)."""
    lib = _analyze_events_protos(load_library())
    rows = np.ascontiguousarray(rows, DETECTION).reshape(-1)
    room = rows.size if cap is None else int(cap)
    out = np.zeros(room, EVENT)
    n = C.c_size_t(0)
    fs = filter._struct(int(n_classes))
    head = (int(device), rows.ctypes.data if rows.size else None, rows.size, int(n_classes), C.addressof(fs))
    answer = (out.ctypes.data if room else None, room, C.byref(n))
    if guards is not None:
        xs = None if extend is None else extend._struct(int(n_classes))
        gs = guards._struct(int(n_classes))
        _check(lib, lib.bnhip_detection_events_guarded(*head, None if xs is None else C.addressof(xs), C.addressof(gs), *answer))
    elif extend is None:
        _check(lib, lib.bnhip_detection_events(*head, *answer))
    else:
        xs = extend._struct(int(n_classes))
        _check(lib, lib.bnhip_detection_events_extended(*head, C.addressof(xs), *answer))
    return out[:n.value] if cap is None else (out[:min(room, n.value)], n.value)


def _event_bank_protos(lib):
    """... and of the real-time event bank and its tick (apart again, for the same reason)."""
    _analyze_events_protos(lib)
    vp, ci, sz = C.c_void_p, C.c_int, C.c_size_t
    answer = [vp, sz, C.POINTER(sz)]                                                  # out, cap, n_out
    lib.bnhip_event_bank_create.argtypes = [ci, ci, ci, ci, vp, C.POINTER(vp)]
    lib.bnhip_event_bank_info.argtypes = [vp] + [C.POINTER(ci)] * 5
    lib.bnhip_event_bank_set_filter.argtypes = [vp, vp]
    lib.bnhip_event_bank_create_extended.argtypes = [ci, ci, ci, ci, vp, vp, C.POINTER(vp)]
    lib.bnhip_event_bank_set_extend.argtypes = [vp, vp]
    lib.bnhip_event_bank_process.argtypes = [vp, vp, ci, vp, vp] + answer
    lib.bnhip_event_bank_process_device.argtypes = [vp, vp, ci, vp, vp] + answer + [vp]
    lib.bnhip_event_bank_flush.argtypes = [vp, ci] + answer
    lib.bnhip_event_bank_reset.argtypes = [vp, ci]
    lib.bnhip_event_bank_pending.argtypes = [vp] + answer
    lib.bnhip_event_bank_clock.argtypes = [vp, ci, C.POINTER(C.c_int64)]
    lib.bnhip_event_bank_destroy.argtypes = [vp]
    lib.bnhip_event_bank_destroy.restype = None
    lib.bnhip_windows_predict_events.argtypes = [vp, vp, vp, ci, ci, C.c_double, ci, C.POINTER(ci), C.POINTER(ci), vp, vp, C.POINTER(vp)] + answer
    lib.bnhip_event_bank_create_dynamic.argtypes = [ci, ci, ci, ci, vp, vp, vp, C.POINTER(vp)]
    lib.bnhip_event_bank_set_dynamic.argtypes = [vp, vp]
    lib.bnhip_event_bank_set_now.argtypes = [vp, C.c_int64]
    lib.bnhip_event_bank_threshold_changes.argtypes = [vp] + answer
    lib.bnhip_event_bank_thresholds.argtypes = [vp] * 6
    lib.bnhip_event_bank_set_thresholds.argtypes = [vp] * 5
    lib.bnhip_event_bank_reset_thresholds.argtypes = [vp, ci]
    lib.bnhip_event_bank_set_guards.argtypes = [vp, vp]
    lib.bnhip_event_bank_set_daylight.argtypes = [vp, ci, vp, ci]
    lib.bnhip_event_threshold.argtypes = [C.c_float, ci, C.c_float]
    lib.bnhip_event_threshold.restype = C.c_float
    return lib


EVENT_PENDING = -1


class EventBank:
    """`bnhip_event_bank` (include/bnhip.h, "Detection events: the real-time bank"): the detection-event rule in streaming form.
    The bank keeps every source's pending detections on the device across calls; `process(sources, conf, idx)` feeds it top-k rows
    (row r is the next window of sources[r]; a source < 0 skips the row) and returns the events (EVENT) that became due, ascending by
    (source, class_index, first_window).  `flush(source=-1)` answers the live events as if the streams had ended, `reset(source=-1)`
    drops them and zeroes the clock, `pending()` lists them with status EVENT_PENDING.  filter: an EventTables; k and its
    hold_windows are fixed for the bank's life.  extend (an EventExtend): the bank is created extended
    (bnhip_event_bank_create_extended) - the hits of its sliding classes move their events' deadlines; `set_extend(extend | None)`
    then changes the table and the numbers, within the longest wait the bank was created with.  A call that fails changes no
    source.  cap: None = whatever the call answers (a call refused for room is repeated with the room it named); a number = that
    room, and HipError with `.needed` beyond it.  dynamic (an EventDynamic): the bank is created dynamic
    (bnhip_event_bank_create_dynamic) - it learns per-class thresholds on the device, at the bank time `set_now(now)` gives;
    `set_dynamic(dynamic | None)` changes the settings or freezes the learning, `thresholds()` / `restore_thresholds(...)` /
    `reset_thresholds(class_index=-1)` are the state's snapshot, restore and reset, and `threshold_changes()` takes the change
    records (THRESHOLD_CHANGE) of the calls since it was last asked.  guards (an EventGuards): `set_guards(guards)` right after
    the create - any bank takes the dog-bark and daylight filters; `set_guards(guards | None)` changes them or turns them off from
    the next call on, and `set_daylight(source, spans)` gives a source its daylight spans [(from, to), ...] in its own clock."""

    ROOM = 256

    def __init__(self, n_classes, k, filter, max_sources=256, device=0, extend=None, dynamic=None, guards=None):
        lib = self._lib = _event_bank_protos(load_library())
        self._h = None
        self.n_classes, self.k, self.max_sources, self.device = int(n_classes), int(k), int(max_sources), int(device)
        self.extended = extend is not None
        fs = filter._struct(self.n_classes)
        h = C.c_void_p()
        self.dynamic = dynamic is not None
        self._changes = []
        if dynamic is not None:
            xs = None if extend is None else extend._struct(self.n_classes)
            ds = dynamic._struct(self.n_classes)
            _check(lib, lib.bnhip_event_bank_create_dynamic(self.device, self.max_sources, self.n_classes, self.k, C.addressof(fs),
                                                            None if xs is None else C.addressof(xs), C.addressof(ds), C.byref(h)))
        elif extend is None:
            _check(lib, lib.bnhip_event_bank_create(self.device, self.max_sources, self.n_classes, self.k, C.addressof(fs), C.byref(h)))
        else:
            xs = extend._struct(self.n_classes)
            _check(lib, lib.bnhip_event_bank_create_extended(self.device, self.max_sources, self.n_classes, self.k, C.addressof(fs), C.addressof(xs),
                                                             C.byref(h)))
        self._h = h
        v = [C.c_int() for _ in range(5)]
        _check(lib, lib.bnhip_event_bank_info(h, *[C.byref(x) for x in v]))
        self.hold_windows, self.slots_per_source = v[3].value, v[4].value
        if guards is not None:
            self.set_guards(guards)

    def set_guards(self, guards):
        """bnhip_event_bank_set_guards: an EventGuards from the next call on (its daylight_spans are not read); None turns them off."""
        gs = None if guards is None else guards._struct(self.n_classes)
        _check(self._lib, self._lib.bnhip_event_bank_set_guards(self._alive(), None if gs is None else C.addressof(gs)))

    def set_daylight(self, source, spans=()):
        """bnhip_event_bank_set_daylight: the daylight spans [(from, to), ...] of a source, in windows of its clock, ascending and
        disjoint, at most EVENT_DAYLIGHT_SPANS; source -1 with no spans clears every source."""
        sp = np.ascontiguousarray(spans, np.int32).reshape(-1, 2)
        _check(self._lib, self._lib.bnhip_event_bank_set_daylight(self._alive(), int(source), sp.ctypes.data if sp.size else None, sp.shape[0]))

    def _alive(self):
        if self._h is None:
            raise HipError(E_INVALID, "event bank is closed")
        return self._h

    def _answer(self, call, cap, changes=True):
        """call(out pointer, room, byref n) -> rc, with the room handled as the class docstring says.  changes: the call replaces the
        bank's change records (process, flush; not pending, after which the previous call's still stand and were collected then)."""
        room = self.ROOM if cap is None else int(cap)
        while True:
            out, n = np.zeros(room, EVENT), C.c_size_t(0)
            rc = call(out.ctypes.data if room else None, room, C.byref(n))
            if rc == E_INVALID and n.value > room:
                if cap is None:
                    room = n.value
                    continue
                msg = (self._lib.bnhip_last_error() or b"").decode("utf-8", "replace")
                e = HipError(rc, msg)
                e.needed = n.value
                raise e
            _check(self._lib, rc)
            if self.dynamic and changes:
                self._collect_changes()
            return out[:n.value]

    def _collect_changes(self):
        """(a dynamic bank, after a successful call) the call's change records join those not yet taken."""
        room = 16
        while True:
            out, n = np.zeros(room, THRESHOLD_CHANGE), C.c_size_t(0)
            rc = self._lib.bnhip_event_bank_threshold_changes(self._alive(), out.ctypes.data, room, C.byref(n))
            if rc == E_INVALID and n.value > room:
                room = n.value
                continue
            _check(self._lib, rc)
            if n.value:
                self._changes.append(out[:n.value])
            return

    def threshold_changes(self):
        """-> the change records (THRESHOLD_CHANGE) of the process / flush / tick calls since the last take, in call order."""
        got, self._changes = self._changes, []
        return np.concatenate(got) if got else np.zeros(0, THRESHOLD_CHANGE)

    def set_now(self, now):
        """bnhip_event_bank_set_now: bank time of the calls that follow; it never decreases."""
        _check(self._lib, self._lib.bnhip_event_bank_set_now(self._alive(), int(now)))

    def set_dynamic(self, dynamic):
        """bnhip_event_bank_set_dynamic: a new EventDynamic from the next call on; None freezes the learning (thr_eff = base)."""
        ds = None if dynamic is None else dynamic._struct(self.n_classes)
        _check(self._lib, self._lib.bnhip_event_bank_set_dynamic(self._alive(), None if ds is None else C.addressof(ds)))

    def thresholds(self):
        """bnhip_event_bank_thresholds -> level, high_count (int32), expires, learned_at (int64), current (float32), [n_classes] each."""
        n = self.n_classes
        a = [np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.float32)]
        _check(self._lib, self._lib.bnhip_event_bank_thresholds(self._alive(), *[x.ctypes.data for x in a]))
        return tuple(a)

    def restore_thresholds(self, level, high_count, expires, learned_at):
        """bnhip_event_bank_set_thresholds: persisted state back into the bank."""
        a = [np.ascontiguousarray(level, np.int32).reshape(-1), np.ascontiguousarray(high_count, np.int32).reshape(-1),
             np.ascontiguousarray(expires, np.int64).reshape(-1), np.ascontiguousarray(learned_at, np.int64).reshape(-1)]
        if any(x.size != self.n_classes for x in a):
            raise HipError(E_INVALID, f"the threshold state holds n_classes = {self.n_classes} entries per array")
        _check(self._lib, self._lib.bnhip_event_bank_set_thresholds(self._alive(), *[x.ctypes.data for x in a]))

    def reset_thresholds(self, class_index=-1):
        _check(self._lib, self._lib.bnhip_event_bank_reset_thresholds(self._alive(), int(class_index)))

    @staticmethod
    def _rows(sources, conf, idx, k):
        src = np.ascontiguousarray(sources, np.int32).reshape(-1)
        conf = np.ascontiguousarray(conf, np.float32).reshape(-1)
        idx = np.ascontiguousarray(idx, np.int32).reshape(-1)
        if conf.size != src.size * k or idx.size != src.size * k:
            raise HipError(E_INVALID, f"the event bank's rows hold k = {k} results")
        return src, conf, idx

    def process(self, sources, conf, idx, cap=None):
        src, conf, idx = self._rows(sources, conf, idx, self.k)
        h, L = self._alive(), self._lib
        P = lambda a: a.ctypes.data if a.size else None
        return self._answer(lambda o, room, n: L.bnhip_event_bank_process(h, P(src), src.size, P(conf), P(idx), o, room, n), cap)

    def flush(self, source=-1, cap=None):
        h, L = self._alive(), self._lib
        return self._answer(lambda o, room, n: L.bnhip_event_bank_flush(h, int(source), o, room, n), cap)

    def pending(self, cap=None):
        h, L = self._alive(), self._lib
        return self._answer(lambda o, room, n: L.bnhip_event_bank_pending(h, o, room, n), cap, changes=False)

    def reset(self, source=-1):
        _check(self._lib, self._lib.bnhip_event_bank_reset(self._alive(), int(source)))

    def set_filter(self, filter):
        fs = filter._struct(self.n_classes)
        _check(self._lib, self._lib.bnhip_event_bank_set_filter(self._alive(), C.addressof(fs)))

    def set_extend(self, extend):
        """bnhip_event_bank_set_extend: a new EventExtend from the next call on; None turns sliding off."""
        xs = None if extend is None else extend._struct(self.n_classes)
        _check(self._lib, self._lib.bnhip_event_bank_set_extend(self._alive(), None if xs is None else C.addressof(xs)))

    def clock(self, source):
        w = C.c_int64(0)
        _check(self._lib, self._lib.bnhip_event_bank_clock(self._alive(), int(source), C.byref(w)))
        return w.value

    def close(self):
        if self._h is not None:
            self._lib.bnhip_event_bank_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _analyze_clips_protos(lib):
    """... and of the detection-clip entries (apart again, for the same reason)."""
    _analyze_events_protos(lib)
    lib.bnhip_event_clip_spans.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.bnhip_recording_clips_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.bnhip_analyze_channels_pcm_clips.argtypes = lib.bnhip_analyze_mixed_pcm.argtypes[:10] + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bnhip_analyze_channels_pcm_clips_extended.argtypes = lib.bnhip_analyze_mixed_pcm.argtypes[:10] + [C.c_void_p] * 5
    lib.bnhip_analyze_channels_pcm_clips_guarded.argtypes = lib.bnhip_analyze_mixed_pcm.argtypes[:10] + [C.c_void_p] * 6
    return lib


# one span of the detection-clip entries (bnhip_clip_span): samples at the model's rate
CLIP_SPAN = np.dtype([("start", "<i8"), ("length", "<i4"), ("recording", "<i4")])


class _ClipExportStruct(C.Structure):
    _fields_ = [("pre_samples", C.c_int32), ("post_samples", C.c_int32), ("max_samples", C.c_int32), ("extended", C.c_int32),
                ("normalize", C.c_int32), ("gate_fallback", C.c_int32), ("target_lufs", C.c_double), ("true_peak_dbtp", C.c_double),
                ("max_gain_db", C.c_double), ("seek_interval", C.c_int32), ("lpc_order", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("rate_out", C.c_int32), ("reserved", C.c_int32), ("window", C.c_void_p), ("top_db", C.c_double),
                ("range_db", C.c_double), ("palette", C.c_void_p)]


class _ClipsOutStruct(C.Structure):
    _fields_ = [("events", C.c_void_p), ("event_cap", C.c_size_t), ("n_events", C.c_size_t), ("spans", C.c_void_p), ("loudness", C.c_void_p),
                ("flac", C.c_void_p), ("flac_cap", C.c_size_t), ("flac_offsets", C.c_void_p), ("png", C.c_void_p), ("png_cap", C.c_size_t),
                ("png_offsets", C.c_void_p), ("n_clips", C.c_size_t)]


class ClipSettings:
    """The export settings of the detection-clip entries (bnhip_clip_export), in samples at the model's rate: the span rule
    (pre_samples, post_samples, max_samples, extended), the normalise (normalize, target_lufs, true_peak_dbtp, max_gain_db,
    gate_fallback), the FLAC encoder (seek_interval, lpc_order) and - with width > 0 and a palette - the spectrogram PNG (width, height
    (default: the one spectrogram_size gives the width), rate_out, window, top_db, range_db).  wav.ClipExport builds one from seconds."""

    def __init__(self, pre_samples, post_samples, max_samples, extended=False, normalize=True, target_lufs=-23.0, true_peak_dbtp=-1.0,
                 max_gain_db=30.0, gate_fallback=False, seek_interval=0, lpc_order=0, width=0, rate_out=0, window=None, top_db=0.0,
                 range_db=100.0, palette=None, height=None):
        self.pre_samples, self.post_samples, self.max_samples, self.extended = int(pre_samples), int(post_samples), int(max_samples), bool(extended)
        self.normalize, self.target_lufs, self.true_peak_dbtp = bool(normalize), float(target_lufs), float(true_peak_dbtp)
        self.max_gain_db, self.gate_fallback = float(max_gain_db), bool(gate_fallback)
        self.seek_interval, self.lpc_order = int(seek_interval), int(lpc_order)
        self.width, self.rate_out, self.top_db, self.range_db = int(width), int(rate_out), float(top_db), float(range_db)
        self.height = (spectrogram_size(self.width)[0] if height is None else int(height)) if self.width > 0 else 0
        self._window = _spectrogram_window(window, 2 * (self.height - 1))[0] if self.width > 0 else None
        self._palette = _png_palette(palette) if self.width > 0 else None

    def _struct(self):
        """-> the C struct (the tables stay alive with self)."""
        return _ClipExportStruct(self.pre_samples, self.post_samples, self.max_samples, int(self.extended), int(self.normalize),
                                 int(self.gate_fallback), self.target_lufs, self.true_peak_dbtp, self.max_gain_db, self.seek_interval,
                                 self.lpc_order, self.width, self.height, self.rate_out, 0,
                                 None if self._window is None else self._window.ctypes.data, self.top_db, self.range_db,
                                 None if self._palette is None else self._palette.ctypes.data)


def event_clip_spans(events, resampled_length, hop, settings):
    """bnhip_event_clip_spans (host only): the clip of every event (EVENT) of recordings of `resampled_length` samples at the model's
    rate, analysed at `hop` -> CLIP_SPAN [n_events]; an event with a non-zero status gets length 0."""
    lib = _analyze_clips_protos(load_library())
    ev = np.ascontiguousarray(events, EVENT).reshape(-1)
    ln = np.ascontiguousarray(resampled_length, np.int64).reshape(-1)
    spans = np.zeros(ev.size, CLIP_SPAN)
    xs = settings._struct()
    _check(lib, lib.bnhip_event_clip_spans(ev.ctypes.data if ev.size else None, ev.size, ln.ctypes.data, ln.size, int(hop), C.addressof(xs),
                                           spans.ctypes.data if ev.size else None))
    return spans


def recording_clips(raw, recs, model_rate, spans, device=0):
    """bnhip_recording_clips_pcm16: the spans (CLIP_SPAN) cut out of recordings (a CHANNELS_RECORDING table; their bytes as the
    channels entries take them) as they are at the model's rate - resampled, and their channel fetched, on the device.
    -> the list of int16 clips of the spans of non-zero length, in span order."""
    lib = _analyze_clips_protos(load_library())
    x, recs = _channels_bytes(raw, recs)
    spans = np.ascontiguousarray(spans, CLIP_SPAN).reshape(-1)
    lens = spans["length"][spans["length"] > 0].astype(np.int64)
    out = np.zeros(max(int(lens.sum()), 1), np.int16)
    _check(lib, lib.bnhip_recording_clips_pcm16(int(device), x.ctypes.data, recs.ctypes.data, recs.size, int(model_rate), spans.ctypes.data,
                                                spans.size, out.ctypes.data))
    ends = np.cumsum(lens)
    return [out[int(e - n):int(e)].copy() for e, n in zip(ends, lens)]


class ClipsResult:
    """What analyze_channels_pcm_clips answers: events (EVENT, the first event_cap), n_events (the total), spans (CLIP_SPAN, one per
    event written), n_clips, and per clip - the j-th span of non-zero length - loudness[j] (Loudness; None without normalize),
    flac[j] (bytes) and png[j] (bytes; png is None without images); chosen as the channels entries answer it."""

    def __init__(self, events, n_events, spans, loudness, flac, png, chosen):
        self.events, self.n_events, self.spans, self.loudness, self.flac, self.png, self.chosen = events, n_events, spans, loudness, flac, png, chosen
        self.n_clips = len(flac)


def _capture_bank_protos(lib):
    """... and of the capture bank (apart again, for the same reason)."""
    _analyze_clips_protos(lib)
    vp, ci, i64 = C.c_void_p, C.c_int, C.c_int64
    lib.bnhip_capture_bank_create.argtypes = [ci, ci, i64, ci, C.POINTER(vp)]
    lib.bnhip_capture_bank_info.argtypes = [vp, C.POINTER(ci), C.POINTER(i64), C.POINTER(ci)]
    lib.bnhip_capture_bank_positions.argtypes = [vp, vp, vp]
    lib.bnhip_capture_bank_reset.argtypes = [vp, ci]
    lib.bnhip_capture_bank_write.argtypes = [vp, ci, vp, vp, vp, ci]
    lib.bnhip_capture_bank_write_levels.argtypes = [vp, vp, ci, vp, vp, vp, vp, ci, vp]
    lib.bnhip_capture_bank_read_pcm16.argtypes = [vp, vp, ci, vp]
    lib.bnhip_capture_bank_clips.argtypes = [vp, vp, ci, vp, vp]
    lib.bnhip_capture_bank_destroy.argtypes = [vp]
    lib.bnhip_capture_bank_destroy.restype = None
    lib.bnhip_capture_spans.argtypes = [vp, C.c_size_t, ci, vp, vp, vp, ci, vp, vp, vp]
    return lib


CAPTURE_OK, CAPTURE_CLAMPED, CAPTURE_NOT_YET, CAPTURE_GONE, CAPTURE_DROPPED = 0, 1, 2, 3, 4

# bnhip_audio_level_data / bnhip_audio_level_stats (include/bnhip.h, "Audio level bank")
AUDIO_LEVEL = np.dtype([("stream", "<i4"), ("frame", "<i4"), ("level", "<i4"), ("clipping", "<i4"), ("n_samples", "<i8"),
                        ("clipped_samples", "<i8"), ("sum_squares", "<u8")])
AUDIO_LEVEL_STATS = np.dtype([("sum", "<i8"), ("count", "<i8"), ("zero_count", "<i8"), ("clip_count", "<i8"), ("min", "<i4"), ("max", "<i4"),
                              ("avg_level", "<i4"), ("zero_pct", "<i4"), ("clipping_pct", "<i4"), ("_pad", "<i4")])


def _pcm_frames(frames, bit_depth, whole):
    """PCM frames (bytes or arrays) of bit_depth -> (uint8 arrays kept alive, int64 sample counts, C array of their addresses) for
    the capture and level bank entries.  A frame that is not whole samples is refused; with whole=False a 16-bit frame of an odd
    byte count loses its last byte instead, as calculateAudioLevel truncates it (buffer_consumer.go:279-287)."""
    size = bit_depth // 8 if bit_depth in (16, 24, 32) else 1
    keep = [np.ascontiguousarray(f).reshape(-1).view(np.uint8) if isinstance(f, np.ndarray) else np.frombuffer(f, np.uint8) for f in frames]
    if not whole and bit_depth == 16:
        keep = [a[:a.size & ~1] for a in keep]
    for a in keep:
        if a.size % size:
            raise HipError(E_INVALID, f"frame of {a.size} bytes is not whole {bit_depth}-bit samples")
    n = np.array([a.size // size for a in keep], np.int64)
    ptr = (C.c_void_p * max(len(keep), 1))(*[a.ctypes.data if a.size else None for a in keep])
    return keep, n, ptr


def capture_spans(events, written, oldest, hop, settings, origins=None):
    """bnhip_capture_spans (host only): the clip of every event (EVENT; `recording` is the source) on the sources' running clocks -
    written / oldest as CaptureBank.positions answers them, origins[s] the position of window 0's first sample (None: 0), hop in
    capture samples -> (CLIP_SPAN [n_events], status int32 [n_events]: CAPTURE_OK, _CLAMPED, _NOT_YET, _GONE or _DROPPED; only the
    first two have a length)."""
    lib = _capture_bank_protos(load_library())
    ev = np.ascontiguousarray(events, EVENT).reshape(-1)
    wr, old = np.ascontiguousarray(written, np.int64).reshape(-1), np.ascontiguousarray(oldest, np.int64).reshape(-1)
    org = None if origins is None else np.ascontiguousarray(origins, np.int64).reshape(-1)
    if old.size != wr.size or (org is not None and org.size != wr.size):
        raise HipError(E_INVALID, "written, oldest and origins hold one entry per source")
    spans, status = np.zeros(ev.size, CLIP_SPAN), np.zeros(ev.size, np.int32)
    xs = settings._struct()
    P = lambda a: a.ctypes.data if ev.size else None
    _check(lib, lib.bnhip_capture_spans(P(ev), ev.size, wr.size, wr.ctypes.data, old.ctypes.data, None if org is None else org.ctypes.data,
                                        int(hop), C.addressof(xs), P(spans), P(status)))
    return spans, status


class CaptureBank:
    """`bnhip_capture_bank` (include/bnhip.h, "Capture bank"): per-source rings of mono int16 on the device - max_sources * capacity * 2
    bytes - written once per tick and cut into detection clips where they lie.  seconds: the least each ring holds (rounded up to
    1024 samples; `capacity` is the result).  Positions are samples on each source's own clock: `written` counts everything given
    since creation or reset, and [oldest, written) is readable."""

    def __init__(self, max_sources, seconds, rate=48000, device=0, capacity_samples=None):
        lib = self._lib = _capture_bank_protos(load_library())
        self._h = None
        self.max_sources, self.rate, self.device = int(max_sources), int(rate), int(device)
        want = int(capacity_samples) if capacity_samples is not None else int(math.ceil(seconds * self.rate))
        h = C.c_void_p()
        _check(lib, lib.bnhip_capture_bank_create(self.device, self.max_sources, want, self.rate, C.byref(h)))
        self._h = h
        cap = C.c_int64()
        _check(lib, lib.bnhip_capture_bank_info(h, None, C.byref(cap), None))
        self.capacity = cap.value

    def _alive(self):
        if self._h is None:
            raise HipError(E_INVALID, "capture bank is closed")
        return self._h

    def write(self, frames, bit_depth=16, levels=None):
        """frames: [(source, PCM bytes or array), ...] - one call per tick for every source; a source may appear several times, its
        frames are appended in call order.  bit_depth 16, 24 or 32: what the bytes hold; the rings keep int16.  levels: (a
        LevelBank, its stream per frame, -1: not measured) - the frames are also measured where the upload has put them
        (bnhip_capture_bank_write_levels) -> the AUDIO_LEVEL records, one per frame."""
        keep, n, ptr = _pcm_frames([f for _, f in frames], bit_depth, whole=True)
        src = np.array([s for s, _ in frames], np.int32)
        if levels is None:
            _check(self._lib, self._lib.bnhip_capture_bank_write(self._alive(), len(keep), src.ctypes.data, n.ctypes.data, ptr, int(bit_depth)))
            return None
        bank, streams = levels
        st = np.array([int(s) for s in streams], np.int32)
        if st.size != len(keep):
            raise HipError(E_INVALID, "levels names one level bank stream per frame")
        out = np.zeros(max(len(keep), 1), AUDIO_LEVEL)
        _check(self._lib, self._lib.bnhip_capture_bank_write_levels(self._alive(), bank._alive(), len(keep), src.ctypes.data, st.ctypes.data,
                                                                    n.ctypes.data, ptr, int(bit_depth), out.ctypes.data))
        return out[:len(keep)]

    def positions(self):
        """-> (written int64 [max_sources], oldest int64 [max_sources])."""
        wr, old = np.zeros(self.max_sources, np.int64), np.zeros(self.max_sources, np.int64)
        _check(self._lib, self._lib.bnhip_capture_bank_positions(self._alive(), wr.ctypes.data, old.ctypes.data))
        return wr, old

    def spans(self, events, hop, settings, origins=None):
        """capture_spans over the bank's positions as they stand."""
        wr, old = self.positions()
        return capture_spans(events, wr, old, hop, settings, origins)

    def read(self, spans):
        """bnhip_capture_bank_read_pcm16: spans (CLIP_SPAN: `recording` the source, `start` a position) -> the list of int16 clips of
        the spans of non-zero length, in span order."""
        spans = np.ascontiguousarray(spans, CLIP_SPAN).reshape(-1)
        lens = spans["length"][spans["length"] > 0].astype(np.int64)
        out = np.zeros(max(int(lens.sum()), 1), np.int16)
        _check(self._lib, self._lib.bnhip_capture_bank_read_pcm16(self._alive(), spans.ctypes.data, spans.size, out.ctypes.data))
        ends = np.cumsum(lens)
        return [out[int(e - n):int(e)].copy() for e, n in zip(ends, lens)]

    def export_raw(self, spans, settings, flac_cap=None, png_cap=None):
        """bnhip_capture_bank_clips -> a ClipsResult without events: the spans as given, and per clip - the j-th span of non-zero
        length - loudness[j], flac[j], png[j].  Room defaults to the bounds of every span."""
        spans = np.ascontiguousarray(spans, CLIP_SPAN).reshape(-1).copy()
        room = spans.size
        lens = [int(n) for n in spans["length"] if n > 0]
        if flac_cap is None:
            flac_cap = flac_ragged_max_bytes(lens, settings.seek_interval) if lens else 0
        if png_cap is None:
            png_cap = png_max_bytes(len(lens), settings.width, settings.height) if lens and settings.width > 0 else 0
        given = np.zeros(max(room, 1), CLIP_SPAN)
        loud = (Loudness * max(room, 1))()
        flac, png = np.empty(max(int(flac_cap), 1), np.uint8), np.empty(max(int(png_cap), 1), np.uint8)
        flac_off, png_off = np.full(room + 1, 2 ** 64 - 1, np.uint64), np.full(room + 1, 2 ** 64 - 1, np.uint64)
        xs = settings._struct()
        o = _ClipsOutStruct(None, 0, 0, given.ctypes.data, C.addressof(loud), flac.ctypes.data, int(flac_cap), flac_off.ctypes.data, png.ctypes.data,
                            int(png_cap), png_off.ctypes.data, 0)
        _check(self._lib, self._lib.bnhip_capture_bank_clips(self._alive(), spans.ctypes.data, spans.size, C.addressof(xs), C.addressof(o)))
        n = int(o.n_clips)
        res = ClipsResult(np.zeros(0, EVENT), 0, given[:room], list(loud[:n]) if settings.normalize else None,
                          _flac_streams(flac, flac_off[:n + 1]) if n else [],
                          (_flac_streams(png, png_off[:n + 1]) if n else []) if settings.width > 0 else None, None)
        res.flac_offsets, res.png_offsets = flac_off, png_off
        return res

    def export(self, spans, settings, flac_cap=None, png_cap=None):
        """The clips of the spans of non-zero length, cut, normalised, encoded and rendered on the device in one call -> one dict per
        clip made: {"flac": bytes, "png": bytes or None, "loudness": Loudness or None, "span": the CLIP_SPAN record}."""
        res = self.export_raw(spans, settings, flac_cap, png_cap)
        made = [q for q in res.spans if q["length"] > 0][:res.n_clips]
        return [{"flac": res.flac[j], "png": res.png[j] if res.png is not None else None,
                 "loudness": res.loudness[j] if res.loudness is not None else None, "span": q} for j, q in enumerate(made)]

    def reset(self, source=-1):
        _check(self._lib, self._lib.bnhip_capture_bank_reset(self._alive(), int(source)))

    def close(self):
        if self._h is not None:
            self._lib.bnhip_capture_bank_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _windows(protos, entry, table, args, resampled=True):
    """The three *_windows entries (host only) over `table` [n] -> (first_window int64 [n + 1], resampled_length int64 [n] or None)."""
    lib = protos(load_library())
    first, n_out = np.zeros(table.size + 1, np.int64), np.zeros(table.size, np.int64) if resampled else None
    w = getattr(lib, entry)(table.ctypes.data if table.size else None, table.size, *[int(v) for v in args], first.ctypes.data,
                            *([n_out.ctypes.data] if resampled else []))
    if w < 0:
        _check(lib, int(w))
    return first, n_out


def analyze_channels_windows(recs, model_rate, n_samples, hop, min_tail=0):
    """bnhip_analyze_channels_windows (host only): analyze_mixed_windows over the (length, rate) of a CHANNELS_RECORDING table."""
    recs = np.ascontiguousarray(recs, CHANNELS_RECORDING).reshape(-1)
    return _windows(_analyze_channels_protos, "bnhip_analyze_channels_windows", recs, (model_rate, n_samples, hop, min_tail))


def channel_energy(raw, recs, device=0):
    """bnhip_channel_energy_pcm: the per-channel measurement behind "auto", alone.  raw: the recordings' interleaved bytes packed back
    to back; recs: a CHANNELS_RECORDING table of integer depths.  -> (CHANNEL_ENERGY [sum of channels], recording-major; chosen int32
    [n]: what "auto" picks).  The exact sum of squares of row i is (int(sum_hi[i]) << 64) | int(sum_lo[i])."""
    lib = _analyze_channels_protos(load_library())
    x, recs = _channels_bytes(raw, recs)
    out = np.zeros(int(recs["channels"].clip(0, None).sum()), CHANNEL_ENERGY)
    chosen = np.zeros(recs.size, np.int32)
    _check(lib, lib.bnhip_channel_energy_pcm(int(device), x.ctypes.data, recs.ctypes.data, recs.size, out.ctypes.data, chosen.ctypes.data))
    return out, chosen


def analyze_mixed_windows(recs, model_rate, n_samples, hop, min_tail=0):
    """bnhip_analyze_mixed_windows (host only): recordings (a RECORDING table) at their own rates, framed at model_rate.
    -> (first_window int64 [n + 1], resampled_length int64 [n]: each recording's samples at model_rate)."""
    recs = np.ascontiguousarray(recs, RECORDING).reshape(-1)
    return _windows(_analyze_mixed_protos, "bnhip_analyze_mixed_windows", recs, (model_rate, n_samples, hop, min_tail))


def analyze_windows(lengths, n_samples, hop, min_tail=0):
    """bnhip_analyze_windows (host only): the window prefix table [n_recordings + 1] of recordings of `lengths` samples framed into
    windows of n_samples advanced by hop; the last entry is the number of windows."""
    ln = np.ascontiguousarray(lengths, np.int64).reshape(-1)
    return _windows(_analyze_protos, "bnhip_analyze_windows", ln, (n_samples, hop, min_tail), resampled=False)[0]


# How a file-analysis call states its recordings: protos / entry - the ctypes prototypes and the entries' common name; x - the checked
# bytes; table - lengths or a recordings table, and args - what the C entries take of it between pcm and hop; windows(n_samples, hop,
# min_tail) -> (first_window, resampled_length); chosen - whether the entries answer a channel per recording
# extra - further arrays the entries fill behind `chosen`, answered behind it
_Form = collections.namedtuple("_Form", "protos entry x table args windows chosen extra", defaults=((),))


def _plain_form(raw, bit_depth, lengths):
    ln = np.ascontiguousarray(lengths, np.int64).reshape(-1)
    x = _checked_bytes(raw, bit_depth, ln, "expected {samples} samples of {bps} bytes")
    return _Form(_analyze_protos, "bnhip_analyze_pcm", x, ln, (bit_depth, ln.ctypes.data, ln.size), lambda *a: (analyze_windows(ln, *a), ln), False)


def _mixed_form(raw, recs, model_rate):
    recs = np.ascontiguousarray(recs, RECORDING).reshape(-1)
    x = _checked_bytes(raw, recs["bits_per_sample"], recs["length"], "the recordings hold {want} bytes")
    return _Form(_analyze_mixed_protos, "bnhip_analyze_mixed_pcm", x, recs, (recs.ctypes.data, recs.size, int(model_rate)),
                 lambda *a: analyze_mixed_windows(recs, model_rate, *a), False)


def _channels_form(raw, recs, model_rate):
    x, recs = _channels_bytes(raw, recs)
    return _Form(_analyze_channels_protos, "bnhip_analyze_channels_pcm", x, recs, (recs.ctypes.data, recs.size, int(model_rate)),
                 lambda *a: analyze_channels_windows(recs, model_rate, *a), True)


def _analyze_flac_protos(lib):
    """... and of the entries for recordings given as FLAC streams (apart again, for the same reason)."""
    _analyze_events_protos(lib)
    head = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_double, C.c_int]
    lib.bnhip_analyze_flac_windows.restype = C.c_longlong
    lib.bnhip_analyze_flac_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
    lib.bnhip_analyze_flac_topk.argtypes = head + [C.c_void_p] * 4
    lib.bnhip_analyze_flac.argtypes = head + [C.c_float, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p]
    lib.bnhip_analyze_flac_events.argtypes = head + [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_void_p]
    return lib


# one stream's verdict of the FLAC entries (bnhip_flac_decode_result)
FLAC_RESULT = np.dtype([("status", "<i4"), ("frames", "<i4"), ("fail_offset", "<u8")])


def analyze_flac_windows(streams, model_rate, n_samples, hop, min_tail=0):
    """bnhip_analyze_flac_windows (host only): analyze_channels_windows over the (length, rate) of FLAC streams' STREAMINFO.
    -> (first_window int64 [n + 1], resampled_length int64 [n])."""
    lib = _analyze_flac_protos(load_library())
    buf, offsets = _flac_burst(streams)
    n = len(streams)
    first, n_out = np.zeros(n + 1, np.int64), np.zeros(n, np.int64)
    w = lib.bnhip_analyze_flac_windows(buf.ctypes.data, offsets.ctypes.data, n, int(model_rate), int(n_samples), int(hop), int(min_tail),
                                       first.ctypes.data, n_out.ctypes.data)
    if w < 0:
        _check(lib, int(w))
    return first, n_out


def _flac_form(streams, select, model_rate):
    """Recordings as a list of FLAC streams; select: one choice for all (a channel index, "mix" or "auto") or one per recording."""
    buf, offsets = _flac_burst(streams)
    n = len(streams)
    sel = np.array([channel_select(s) for s in (select if isinstance(select, (list, tuple, np.ndarray)) else [select] * n)], np.int32)
    if sel.size != n:
        raise HipError(E_INVALID, "select holds one choice per recording")
    form = _Form(_analyze_flac_protos, "bnhip_analyze_flac", buf, sel, (offsets.ctypes.data, sel.ctypes.data, n, int(model_rate)),
                 lambda *a: analyze_flac_windows(streams, model_rate, *a), True, (np.zeros(n, FLAC_RESULT),))
    return form, offsets                                # (offsets: kept alive by the caller for the call)


# How such a call is answered: (lib, kk = min(k, n_classes), first() -> first_window, room(cap) -> records to make room for) -> (the
# entry's suffix, the C arguments behind k, result() -> what the call returns, as a tuple)
def _topk_answer():
    def answer(lib, kk, first, room):
        f = first()
        conf, idx = np.empty((int(f[-1]), kk), np.float32), np.empty((int(f[-1]), kk), np.int32)
        return "_topk", (conf.ctypes.data, idx.ctypes.data), lambda: (conf, idx, f)
    return answer


def _rows_answer(threshold, cap):
    def answer(lib, kk, first, room):
        rows, n = np.zeros(room(cap), DETECTION), C.c_size_t(0)
        return "", (float(threshold), rows.ctypes.data if rows.size else None, rows.size, C.byref(n)), lambda: (rows[:min(rows.size, n.value)], n.value)
    return answer


def _events_answer(filter, cap, n_classes, extend=None, guards=None):
    """extend (an EventExtend): the _events_extended entry, which only the channels form has; guards (an EventGuards): its
    _events_guarded entry, under the extend or none."""
    def answer(lib, kk, first, room):
        _analyze_events_protos(lib)
        first()                                         # (a bad table is answered as the windows entry answers it, before the filter)
        out, n, fs = np.zeros(room(cap), EVENT), C.c_size_t(0), filter._struct(n_classes)
        xs = None if extend is None else extend._struct(n_classes)
        gs = None if guards is None else guards._struct(n_classes)
        middle = (() if xs is None else (C.byref(xs),)) if gs is None else (None if xs is None else C.byref(xs), C.byref(gs))
        return "_events_guarded" if gs is not None else "_events" if xs is None else "_events_extended", \
            (C.byref(fs),) + middle + (out.ctypes.data if out.size else None, out.size, C.byref(n)), \
            lambda: (out[:n.value],) if cap is None else (out[:min(out.size, n.value)], n.value)
    return answer


def init():
    """-> number of devices (InitOV analogue, backend_openvino.go:477)."""
    lib = load_library()
    n = C.c_int(0)
    _check(lib, lib.bnhip_init(C.byref(n)))
    return n.value


class PinnedArray:
    """A numpy array over page-locked memory from bnhip_host_alloc (the reference's shim keeps a C-allocated input buffer per
    classifier, backend_openvino.go:673-680): bnhip_predict* read / write such buffers by DMA, without the staging copy.
    `.array` is the view; free() (or the with-statement) releases it.  The memory is C-owned: views or slices of `.array` taken
    before free() dangle afterwards (numpy cannot know) - copy what must outlive it, and never free() during a predict call."""

    def __init__(self, shape, dtype=np.float32):
        self._lib = load_library()
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self._lib.bnhip_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
        _check(self._lib, self._lib.bnhip_host_alloc(n, C.byref(p)))          # (zero bytes: BNHIP_E_INVALID)
        self._p = p
        buf = (C.c_char * n).from_address(p.value)
        self.array = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def free(self):
        if self._p:
            self.array = None
            self._lib.bnhip_host_free.argtypes = [C.c_void_p]
            self._lib.bnhip_host_free(self._p)
            self._p = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


class HipClassifier:
    """inference.Classifier + EmbeddingExtractor over libbnhip.so.  NOT thread-safe (backend.go:7)."""

    def __init__(self, model_bytes: bytes, device=0, max_batch=256, plan_only=False, debug_no_reuse=False,
                 graphs=None, frontend_fft=None, depth=None, lanes=None, autotune=None, devices=None, replicate=None,
                 bf16x3=None, precision=None, logits_output=None, embedding_output=None, host_depth=None, tune_dir=None):
        self._lib = load_library()
        self._h = C.c_void_p()
        o = {"device": device, "max_batch": max_batch, "plan_only": int(plan_only), "debug_no_reuse": int(debug_no_reuse)}
        if devices is not None:          # one handle sharding every call over several GPUs (bnhip.h "devices")
            o["devices"] = [int(d) for d in devices]
        if replicate is not None:
            o["replicate"] = str(replicate)
        if bf16x3 is not None:
            o["bf16x3"] = int(bf16x3)
        if logits_output is not None:    # graph output indices (default: the reference's per-family rule, bnhip.h)
            o["logits_output"] = int(logits_output)
        if embedding_output is not None:
            o["embedding_output"] = int(embedding_output)
        if precision is not None:        # "f32" (default) | "bf16": MFMA operands rounded to bf16, fp32 accumulate (Perch-style)
            o["precision"] = str(precision)
        if graphs is not None:
            o["graphs"] = int(graphs)
        if frontend_fft is not None:
            o["frontend_fft"] = int(frontend_fft)
        if depth is not None:
            o["depth"] = int(depth)
        if host_depth is not None:       # contexts the blocking host-pointer entries pipeline their chunks over (default 2)
            o["host_depth"] = int(host_depth)
        if lanes is not None:
            o["lanes"] = int(lanes)
        if autotune is not None:
            o["autotune"] = int(autotune)
        # recorded tunings (bnhip.h "tune_dir"): the package's own directory unless the caller or BNHIP_TUNE_DIR says otherwise
        # ("" = none: always time the candidates)
        if tune_dir is None and "BNHIP_TUNE_DIR" not in os.environ and os.path.isdir(TUNE_DIR):
            tune_dir = TUNE_DIR
        if tune_dir:
            o["tune_dir"] = str(tune_dir)
        opts = json.dumps(o).encode()
        buf = (C.c_char * len(model_bytes)).from_buffer_copy(model_bytes)
        _check(self._lib, self._lib.bnhip_model_create(C.cast(buf, C.c_void_p), len(model_bytes), opts, C.byref(self._h)))
        ns, nc, ed = C.c_int(), C.c_int(), C.c_int()
        _check(self._lib, self._lib.bnhip_model_info(self._h, C.byref(ns), C.byref(nc), C.byref(ed)))
        self.n_samples, self._n_classes, self.emb_dim = ns.value, nc.value, ed.value
        self.max_batch = max_batch

    # ---- inference.Classifier
    def predict(self, samples):
        """Predict(samples []float32) ([]float32, error): raw logits for ONE clip."""
        x = np.ascontiguousarray(samples, np.float32).reshape(-1)
        if x.size != self.n_samples:
            raise HipError(E_INVALID, f"input size mismatch: expected {self.n_samples} samples, got {x.size}")
        return self.predict_batch(x, 1)[0]

    def num_species(self):
        return self._n_classes

    def close(self):
        if self._h:
            self._lib.bnhip_model_destroy(self._h)
            self._h = C.c_void_p()

    # ---- inference.EmbeddingExtractor
    def predict_with_embeddings(self, samples):
        x = np.ascontiguousarray(samples, np.float32).reshape(-1)
        if x.size != self.n_samples:
            raise HipError(E_INVALID, f"input size mismatch: expected {self.n_samples} samples, got {x.size}")
        if not self.emb_dim:
            return self.predict(x), None
        lg, em = self.predict_batch(x, 1, want_embeddings=True)
        return lg[0], em[0]

    # ---- onnx.Classifier.PredictBatch shape: flat [B*N] in, [B, classes] out
    def predict_batch(self, flat, batch_size, want_embeddings=False, out=None):
        """`out`: optional preallocated float32 [batch_size, classes] result array (a serving loop reuses it; a fresh
        numpy array costs a page fault per 4 KB on its first write)."""
        self._alive()
        x = np.ascontiguousarray(flat, np.float32).reshape(-1)
        if batch_size <= 0 or x.size != batch_size * self.n_samples:
            raise HipError(E_INVALID, f"input size mismatch: expected {batch_size * self.n_samples} samples, got {x.size}")
        logits = self._out(out, batch_size)
        emb = np.empty((batch_size, self.emb_dim), np.float32) if (want_embeddings and self.emb_dim) else None
        _check(self._lib, self._lib.bnhip_predict(self._h, x.ctypes.data, batch_size, logits.ctypes.data,
                                                  emb.ctypes.data if emb is not None else None))
        return (logits, emb) if want_embeddings else logits

    def _out(self, out, batch_size):
        if out is None:
            return np.empty((batch_size, self._n_classes), np.float32)
        if out.dtype != np.float32 or not out.flags.c_contiguous or out.size != batch_size * self._n_classes:
            raise HipError(E_INVALID, "out must be a C-contiguous float32 array of batch_size * classes elements")
        return out.reshape(batch_size, self._n_classes)

    def predict_pcm16(self, pcm, batch_size, out=None):
        self._alive()
        x = np.ascontiguousarray(pcm, np.int16).reshape(-1)
        if x.size != batch_size * self.n_samples:
            raise HipError(E_INVALID, f"input size mismatch: expected {batch_size * self.n_samples} samples, got {x.size}")
        logits = self._out(out, batch_size)
        _check(self._lib, self._lib.bnhip_predict_pcm16(self._h, x.ctypes.data, batch_size, logits.ctypes.data, None))
        return logits

    def predict_pcm(self, raw: bytes, bit_depth: int, batch_size: int):
        """Little-endian PCM bytes of the three depths ConvertToFloat32 accepts (convert/pcm.go:206-268), converted on the
        device.  An unsupported depth is a validation error, as in the reference (pcm.go:215-222)."""
        self._alive()
        if bit_depth not in (16, 24, 32):
            raise HipError(E_INVALID, f"unsupported bit depth: {bit_depth} (supported: 16, 24, 32)")
        x = np.frombuffer(raw, np.uint8)
        if x.size != batch_size * self.n_samples * (bit_depth // 8):
            raise HipError(E_INVALID, f"input size mismatch: expected {batch_size * self.n_samples} samples of "
                                      f"{bit_depth // 8} bytes, got {x.size} bytes")
        logits = np.empty((batch_size, self._n_classes), np.float32)
        _check(self._lib, self._lib.bnhip_predict_pcm(self._h, x.ctypes.data, bit_depth, batch_size, logits.ctypes.data, None))
        return logits

    def predict_device(self, d_samples_ptr, n_clips, d_logits_ptr, d_emb_ptr=None):
        self._alive()
        _check(self._lib, self._lib.bnhip_predict_device(self._h, d_samples_ptr, n_clips, d_logits_ptr, d_emb_ptr))

    def postprocess_topk(self, logits, k=10, activation=0, sensitivity=1.0):
        self._alive()
        lg = np.ascontiguousarray(logits, np.float32).reshape(-1, self._n_classes)
        kk = min(k, self._n_classes)
        conf = np.empty((lg.shape[0], kk), np.float32)
        idx = np.empty((lg.shape[0], kk), np.int32)
        _check(self._lib, self._lib.bnhip_postprocess_topk(self._h, lg.ctypes.data, lg.shape[0], self._n_classes,
                                                           activation, sensitivity, k, conf.ctypes.data, idx.ctypes.data))
        return conf, idx

    def predict_topk(self, flat, batch_size, k=10, activation=0, sensitivity=1.0):
        self._alive()
        x = np.ascontiguousarray(flat, np.float32).reshape(-1)
        if x.size != batch_size * self.n_samples:
            raise HipError(E_INVALID, f"input size mismatch: expected {batch_size * self.n_samples} samples, got {x.size}")
        kk = min(k, self._n_classes)
        conf = np.empty((batch_size, kk), np.float32)
        idx = np.empty((batch_size, kk), np.int32)
        _check(self._lib, self._lib.bnhip_predict_topk(self._h, x.ctypes.data, batch_size, activation, sensitivity, k,
                                                       conf.ctypes.data, idx.ctypes.data))
        return conf, idx

    def predict_pcm_topk(self, raw, bit_depth, batch_size, k=10, activation=0, sensitivity=1.0):
        """predict_pcm + postprocess_topk in one call (bnhip_predict_pcm_topk): the windows' PCM bytes in, top-k out; neither the
        float samples nor the logits exist on the host."""
        self._alive()
        if bit_depth not in (16, 24, 32):
            raise HipError(E_INVALID, f"unsupported bit depth: {bit_depth} (supported: 16, 24, 32)")
        x = np.frombuffer(raw, np.uint8)
        if x.size != batch_size * self.n_samples * (bit_depth // 8):
            raise HipError(E_INVALID, f"input size mismatch: expected {batch_size * self.n_samples} samples of "
                                      f"{bit_depth // 8} bytes, got {x.size} bytes")
        kk = min(k, self._n_classes)
        conf = np.empty((batch_size, kk), np.float32)
        idx = np.empty((batch_size, kk), np.int32)
        _check(self._lib, self._lib.bnhip_predict_pcm_topk(self._h, x.ctypes.data, bit_depth, batch_size, activation, sensitivity, k,
                                                           conf.ctypes.data, idx.ctypes.data))
        return conf, idx

    def predict_windows_events(self, win, bank, bit_depth=16, k=10, activation=0, sensitivity=1.0):
        """One tick answered as rows and as detection events (bnhip_windows_predict_events): every ready window of the assembler
        `win` (stream.NativeWindows) through the model, the top-k rows back as bnhip_windows_predict_topk writes them, and in the same
        call fed to `bank` (an EventBank on this device; its source numbers are the assembler's).
        -> (source indices, rows view, conf [n, kk], idx [n, kk], events)."""
        return win.predict_events(self, bank, bit_depth, k, activation, sensitivity)

    def _room(self, cap, first, k):
        """Records a file-analysis call makes room for: every row (an event is made of at least one) unless cap says less."""
        return int(first()[-1]) * min(k, self._n_classes) if cap is None else int(cap)

    def _analyze(self, form, answer, hop, min_tail, k, activation, sensitivity):
        """The body of the nine analyze_* calls: the recordings as `form` states them (a _Form), answered as `answer` says."""
        self._alive()
        lib = form.protos(self._lib)
        table = []                                      # the window table, made when the answer first asks for it

        def first():
            if not table:
                table.append(form.windows(self.n_samples, hop, min_tail)[0])
            return table[0]
        suffix, tail, result = answer(lib, min(k, self._n_classes), first, lambda cap: self._room(cap, first, k))
        chosen = ([np.zeros(form.table.size, np.int32)] if form.chosen else []) + list(form.extra)
        _check(lib, getattr(lib, form.entry + suffix)(self._h, form.x.ctypes.data, *form.args, int(hop), int(min_tail), activation, sensitivity, k,
                                                      *tail, *[c.ctypes.data for c in chosen]))
        got = result() + tuple(chosen)
        return got[0] if len(got) == 1 else got

    def analyze_pcm_topk(self, raw, bit_depth, lengths, hop, min_tail=0, k=10, activation=0, sensitivity=1.0):
        """bnhip_analyze_pcm_topk: recordings (packed back to back, `lengths` samples each; bit_depth 0 = float32) in, the top-k of
        every overlapping window out - the windows are framed on the device.  -> (conf [W, k], idx [W, k], first_window)."""
        return self._analyze(_plain_form(raw, bit_depth, lengths), _topk_answer(), hop, min_tail, k, activation, sensitivity)

    def analyze_pcm(self, raw, bit_depth, lengths, hop, min_tail=0, k=10, activation=0, sensitivity=1.0, threshold=0.0, cap=None):
        """bnhip_analyze_pcm: the same call, answered as detection rows (DETECTION: recording, window inside the recording,
        class_index, confidence) with confidence >= threshold, ordered by window, then rank.  -> (rows, total); cap limits the rows
        written (default: room for every row), total is their number whatever the cap."""
        return self._analyze(_plain_form(raw, bit_depth, lengths), _rows_answer(threshold, cap), hop, min_tail, k, activation, sensitivity)

    def analyze_mixed_pcm_topk(self, raw, recs, model_rate, hop, min_tail=0, k=10, activation=0, sensitivity=1.0):
        """bnhip_analyze_mixed_pcm_topk: recordings at their own rates and depths (a RECORDING table; their bytes packed back to
        back as they are in their files) in, the top-k of every overlapping window at model_rate out - resampled, converted and
        framed on the device.  hop and min_tail count samples at model_rate.  -> (conf [W, k], idx [W, k], first_window)."""
        return self._analyze(_mixed_form(raw, recs, model_rate), _topk_answer(), hop, min_tail, k, activation, sensitivity)

    def analyze_mixed_pcm(self, raw, recs, model_rate, hop, min_tail=0, k=10, activation=0, sensitivity=1.0, threshold=0.0, cap=None):
        """bnhip_analyze_mixed_pcm: the same call, answered as detection rows, as analyze_pcm answers.  -> (rows, total)."""
        return self._analyze(_mixed_form(raw, recs, model_rate), _rows_answer(threshold, cap), hop, min_tail, k, activation, sensitivity)

    def analyze_channels_pcm_topk(self, raw, recs, model_rate, hop, min_tail=0, k=10, activation=0, sensitivity=1.0):
        """bnhip_analyze_channels_pcm_topk: multichannel recordings (a CHANNELS_RECORDING table; their interleaved frames packed
        back to back as they are in their files) in; each recording's chosen channel, or the mean of its channels, is what
        analyze_mixed_pcm_topk then analyses - fetched, and where asked decided, on the device.
        -> (conf [W, k], idx [W, k], first_window, chosen int32 [n]: the channel read or CHANNEL_MIX)."""
        return self._analyze(_channels_form(raw, recs, model_rate), _topk_answer(), hop, min_tail, k, activation, sensitivity)

    def analyze_channels_pcm(self, raw, recs, model_rate, hop, min_tail=0, k=10, activation=0, sensitivity=1.0, threshold=0.0, cap=None):
        """bnhip_analyze_channels_pcm: the same call, answered as detection rows, as analyze_pcm answers.  -> (rows, total, chosen)."""
        return self._analyze(_channels_form(raw, recs, model_rate), _rows_answer(threshold, cap), hop, min_tail, k, activation, sensitivity)

    def analyze_flac_topk(self, streams, select, model_rate, hop, min_tail=0, k=10, activation=0, sensitivity=1.0):
        """bnhip_analyze_flac_topk: analyze_channels_pcm_topk with the recordings given as FLAC streams (a list of bytes; 1 or 2
        channels, 16 or 24 bits) - rate, depth, channels and length are STREAMINFO's, the compressed bytes go up once and are decoded
        on the device.  select: a channel index, "mix" or "auto", for all or per recording.
        -> (conf, idx, first_window, chosen, results: a FLAC_RESULT per recording - a damaged stream does not fail the call)."""
        form, keep = _flac_form(streams, select, model_rate)
        return self._analyze(form, _topk_answer(), hop, min_tail, k, activation, sensitivity)

    def analyze_flac(self, streams, select, model_rate, hop, min_tail=0, k=10, activation=0, sensitivity=1.0, threshold=0.0, cap=None):
        """bnhip_analyze_flac: the same call, answered as detection rows.  -> (rows, total, chosen, results)."""
        form, keep = _flac_form(streams, select, model_rate)
        return self._analyze(form, _rows_answer(threshold, cap), hop, min_tail, k, activation, sensitivity)

    def analyze_flac_events(self, streams, select, model_rate, hop, filter, min_tail=0, k=10, activation=0, sensitivity=1.0, cap=None):
        """bnhip_analyze_flac_events: the same call, answered as detection events.  -> (events, chosen, results); with cap ->
        (events[:cap], total, chosen, results)."""
        form, keep = _flac_form(streams, select, model_rate)
        return self._analyze(form, _events_answer(filter, cap, self._n_classes), hop, min_tail, k, activation, sensitivity)

    def analyze_pcm_events(self, raw, bit_depth, lengths, hop, filter, min_tail=0, k=10, activation=0, sensitivity=1.0, cap=None):
        """bnhip_analyze_pcm_events: the analyze_pcm call answered as detection events (EVENT) - the rows merged on the device under
        `filter` (an EventTables).  -> the events, ascending by (recording, class_index, first_window); with cap -> (events[:cap], total)."""
        return self._analyze(_plain_form(raw, bit_depth, lengths), _events_answer(filter, cap, self._n_classes), hop, min_tail, k, activation, sensitivity)

    def analyze_mixed_pcm_events(self, raw, recs, model_rate, hop, filter, min_tail=0, k=10, activation=0, sensitivity=1.0, cap=None):
        """bnhip_analyze_mixed_pcm_events: analyze_mixed_pcm answered as detection events, as analyze_pcm_events answers."""
        return self._analyze(_mixed_form(raw, recs, model_rate), _events_answer(filter, cap, self._n_classes), hop, min_tail, k, activation, sensitivity)

    def analyze_channels_pcm_events(self, raw, recs, model_rate, hop, filter, min_tail=0, k=10, activation=0, sensitivity=1.0, cap=None,
                                    extend=None, guards=None):
        """bnhip_analyze_channels_pcm_events: analyze_channels_pcm answered as detection events; with extend (an EventExtend)
        bnhip_analyze_channels_pcm_events_extended; with guards (an EventGuards) bnhip_analyze_channels_pcm_events_guarded, under
        the extend or none.  -> (events, chosen); with cap -> (events[:cap], total, chosen)."""
        return self._analyze(_channels_form(raw, recs, model_rate), _events_answer(filter, cap, self._n_classes, extend, guards), hop, min_tail, k,
                             activation, sensitivity)

    def analyze_channels_pcm_clips(self, raw, recs, model_rate, hop, filter, settings, min_tail=0, k=10, activation=0, sensitivity=1.0,
                                   event_cap=None, max_clips=None, flac_cap=None, png_cap=None, extend=None, guards=None):
        """bnhip_analyze_channels_pcm_clips (with extend, an EventExtend: bnhip_analyze_channels_pcm_clips_extended; with guards, an
        EventGuards: bnhip_analyze_channels_pcm_clips_guarded, under the extend or none):
        analyze_channels_pcm_events, and in the same call the clip of every event written - cut
        out of the recordings on the device, normalised, FLAC-encoded and (with settings.width) rendered to a PNG - under `settings`
        (a ClipSettings).  Room: event_cap events (default: every row), and for the streams flac_cap / png_cap bytes (default: the
        bounds of max_clips clips of the longest span the settings allow; max_clips defaults to min(event_cap, 65535)).  Clips are
        made in event order for as long as their bounds fit.  -> a ClipsResult; its flac_offsets / png_offsets are the raw uint64
        tables [event_cap + 1], untouched (all ones) from n_clips + 1 on."""
        self._alive()
        _analyze_clips_protos(self._lib)
        form = _channels_form(raw, recs, model_rate)
        first, n_out = form.windows(self.n_samples, hop, min_tail)
        room = self._room(event_cap, lambda: first, k)
        n_max = min(room, 65535) if max_clips is None else int(max_clips)
        longest = max(1, min(settings.max_samples, int(n_out.max())))
        if not settings.extended:
            longest = max(1, min(longest, settings.pre_samples + settings.post_samples))
        if flac_cap is None:
            flac_cap = flac_ragged_max_bytes([longest] * n_max, settings.seek_interval) if n_max else 0
        if png_cap is None:
            png_cap = png_max_bytes(n_max, settings.width, settings.height) if n_max and settings.width > 0 else 0
        events, spans = np.zeros(room, EVENT), np.zeros(room, CLIP_SPAN)
        loud = (Loudness * max(room, 1))()
        flac, png = np.empty(max(int(flac_cap), 1), np.uint8), np.empty(max(int(png_cap), 1), np.uint8)
        flac_off, png_off = np.full(room + 1, 2 ** 64 - 1, np.uint64), np.full(room + 1, 2 ** 64 - 1, np.uint64)
        chosen = np.zeros(form.table.size, np.int32)
        fs, xs = filter._struct(self._n_classes), settings._struct()
        o = _ClipsOutStruct(events.ctypes.data, room, 0, spans.ctypes.data, C.addressof(loud), flac.ctypes.data, int(flac_cap), flac_off.ctypes.data,
                            png.ctypes.data, int(png_cap), png_off.ctypes.data, 0)
        head = (self._h, form.x.ctypes.data, *form.args, int(hop), int(min_tail), activation, sensitivity, k, C.addressof(fs))
        if guards is not None:
            es = None if extend is None else extend._struct(self._n_classes)
            gs = guards._struct(self._n_classes)
            _check(self._lib, self._lib.bnhip_analyze_channels_pcm_clips_guarded(*head, None if es is None else C.addressof(es), C.addressof(gs),
                                                                                 chosen.ctypes.data, C.addressof(xs), C.addressof(o)))
        elif extend is None:
            _check(self._lib, self._lib.bnhip_analyze_channels_pcm_clips(*head, chosen.ctypes.data, C.addressof(xs), C.addressof(o)))
        else:
            es = extend._struct(self._n_classes)
            _check(self._lib, self._lib.bnhip_analyze_channels_pcm_clips_extended(*head, C.addressof(es), chosen.ctypes.data, C.addressof(xs),
                                                                                  C.addressof(o)))
        n_ev, n = min(room, o.n_events), int(o.n_clips)
        res = ClipsResult(events[:n_ev], int(o.n_events), spans[:n_ev], list(loud[:n]) if settings.normalize else None,
                          _flac_streams(flac, flac_off[:n + 1]) if n else [],
                          (_flac_streams(png, png_off[:n + 1]) if n else []) if settings.width > 0 else None, chosen)
        res.flac_offsets, res.png_offsets = flac_off, png_off
        return res

    # ---- plumbing
    def set_stream(self, hip_stream_ptr):
        _check(self._lib, self._lib.bnhip_set_stream(self._h, hip_stream_ptr))

    def synchronize(self):
        _check(self._lib, self._lib.bnhip_synchronize(self._h))

    def profile_enable(self, on=True):
        _check(self._lib, self._lib.bnhip_profile_enable(self._h, int(on)))

    def profile_filter(self, kernel_class=None):
        _check(self._lib, self._lib.bnhip_profile_filter(self._h, kernel_class.encode() if kernel_class else None))

    def profile_read(self, per_step=False):
        """Per-kernel-class timing rows; with per_step=True returns (classes, steps)."""
        buf = C.create_string_buffer(1 << 18)
        rc = self._lib.bnhip_profile_read(self._h, buf, len(buf))
        if rc < 0:
            _check(self._lib, rc)
        rows = json.loads(buf.value.decode())
        classes = [r for r in rows if "step" not in r]
        return (classes, [r for r in rows if "step" in r]) if per_step else classes

    def profile_steps(self, on=True):
        _check(self._lib, self._lib.bnhip_profile_steps(self._h, int(on)))

    def profile_steps_read(self, cap=4096):
        """(start_ms, end_ms) of every call since the last read, relative to the first call's start."""
        a, b = np.zeros(cap, np.float64), np.zeros(cap, np.float64)
        lib = self._lib
        lib.bnhip_profile_steps_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        n = lib.bnhip_profile_steps_read(self._h, a.ctypes.data, b.ctypes.data, cap)
        if n < 0:
            _check(lib, n)
        n = min(n, cap)
        return a[:n].copy(), b[:n].copy()

    def describe(self):
        need = self._lib.bnhip_model_describe(self._h, None, 0)
        if need < 0:
            _check(self._lib, need)
        buf = C.create_string_buffer(need + 16)
        self._lib.bnhip_model_describe(self._h, buf, len(buf))
        return json.loads(buf.value.decode())

    def debug_fetch(self, tensor_index, n_clips, max_floats_per_clip):
        out = np.empty(n_clips * max_floats_per_clip, np.float32)
        lib = self._lib
        lib.bnhip_debug_fetch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        rc = lib.bnhip_debug_fetch(self._h, tensor_index, n_clips, out.ctypes.data, out.size)
        if rc < 0:
            _check(lib, rc)
        return out[:rc * n_clips].reshape(n_clips, rc)

    def _alive(self):
        if not self._h:
            raise HipError(E_INVALID, "classifier is closed")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def us_frame_cv(samples, sample_rate, fft_size=8192, hop=4096, split_hz=20000, device=0):
    """ultrasonic.ComputeUSFrameCV (filter.go:20) for a batch: samples [B, n] float64 -> (cv[B], ok[B])."""
    lib = load_library()
    s = np.ascontiguousarray(samples, np.float64)
    if s.ndim == 1:
        s = s[None, :]
    cv = np.zeros(s.shape[0], np.float64)
    ok = np.zeros(s.shape[0], np.int32)
    _check(lib, lib.bnhip_us_frame_cv(device, s.ctypes.data, s.shape[0], s.shape[1], sample_rate, fft_size, hop,
                                      split_hz, cv.ctypes.data, ok.ctypes.data))
    return cv, ok.astype(bool)


def spectrogram_size(width):
    """-> (height, fft_size) of a `width`-pixel image: fftFriendlyHeight (spectrogram/generator.go:115-123) and N = 2 (height - 1)."""
    lib = load_library()
    lib.bnhip_spectrogram_size.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    h, n = C.c_int(0), C.c_int(0)
    _check(lib, lib.bnhip_spectrogram_size(int(width), C.byref(h), C.byref(n)))
    return h.value, n.value


def _spectrogram_window(window, fft_size):
    """(keep-alive array, pointer) of a caller's window table; None -> NULL (periodic Hann on the host side of the C ABI)."""
    if window is None:
        return None, None
    w = np.ascontiguousarray(window, np.float64)
    if w.shape != (fft_size,):
        raise HipError(E_INVALID, f"window must hold {fft_size} coefficients, got shape {w.shape}")
    return w, w.ctypes.data


def spectrogram(clips_pcm16, rate, width, rate_out=0, window=None, top_db=0.0, range_db=100.0, device=0):
    """Raw spectrogram images of a batch of equally long clips in one device call (what GenerateFromPCM, spectrogram/generator.go:425,
    asks sox for clip by clip): int16 [B, n] (or [n]) at `rate` Hz -> uint8 [B, H, W] level indices, Nyquist in row 0.
    rate_out: resample first (24 000 bird profile, 256 000 bat profile); 0 renders at the source rate.  Spec: DESIGN.md §9."""
    lib = load_library()
    x = np.ascontiguousarray(clips_pcm16, np.int16)
    if x.ndim == 1:
        x = x[None, :]
    if x.ndim != 2 or x.shape[0] == 0 or x.shape[1] == 0:
        raise HipError(E_INVALID, "clips must be a non-empty int16 [B, n] array")
    height, fft_size = spectrogram_size(width)
    keep, wp = _spectrogram_window(window, fft_size)
    img = np.empty((x.shape[0], height, int(width)), np.uint8)
    lib.bnhip_spectrogram_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_double, C.c_double, C.c_void_p]
    _check(lib, lib.bnhip_spectrogram_pcm16(device, x.ctypes.data, x.shape[0], x.shape[1], int(rate), int(rate_out), int(width), height,
                                            wp, float(top_db), float(range_db), img.ctypes.data))
    del keep
    return img


def spectrogram_device(d_samples_ptr, f32, n_clips, n, width, height, d_image_ptr, window=None, top_db=0.0, range_db=100.0, device=0,
                       hip_stream_ptr=None):
    """Device-resident form: samples (int16, or float32 with f32) and the uint8 [n_clips, height, width] image are device pointers;
    enqueued on the stream, not synchronised."""
    lib = load_library()
    keep, wp = _spectrogram_window(window, 2 * (int(height) - 1))
    lib.bnhip_spectrogram_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double,
                                             C.c_double, C.c_void_p, C.c_void_p]
    _check(lib, lib.bnhip_spectrogram_device(device, d_samples_ptr, 1 if f32 else 0, int(n_clips), int(n), int(width), int(height), wp,
                                             float(top_db), float(range_db), d_image_ptr, hip_stream_ptr))
    del keep


LOUDNESS_PEAK_LIMITED, LOUDNESS_GATE_LIFTED, LOUDNESS_CLAMPED = 1, 2, 4


class Loudness(C.Structure):
    """bnhip_loudness: one clip's measurement, plan and flags (bnhip.h)."""
    _fields_ = [("integrated_lufs", C.c_double), ("true_peak_dbtp", C.c_double), ("true_peak", C.c_double),
                ("target_gain_db", C.c_double), ("lift_db", C.c_double), ("planned_gain_db", C.c_double), ("gain_db", C.c_double),
                ("factor", C.c_double), ("output_lufs", C.c_double), ("flags", C.c_int), ("reserved", C.c_int)]

    @property
    def peak_limited(self):
        return bool(self.flags & LOUDNESS_PEAK_LIMITED)

    @property
    def gate_lifted(self):
        return bool(self.flags & LOUDNESS_GATE_LIFTED)

    @property
    def clamped(self):
        return bool(self.flags & LOUDNESS_CLAMPED)


def _mono_pcm16_clips(what, clips_pcm16, channels):
    """int16 [B, n] of a batch (or one clip [n]) for the `what` entries ("loudness", "FLAC"); anything but mono int16 is
    BNHIP_E_UNSUPPORTED (conf.NumChannels is 1)."""
    if int(channels) != 1:
        raise HipError(E_UNSUPPORTED, f"{what} entries are mono, got {channels} channels")
    x = np.ascontiguousarray(clips_pcm16)
    if x.dtype != np.int16:
        raise HipError(E_UNSUPPORTED, f"{what} entries take int16 PCM, got {x.dtype}")
    if x.ndim == 1:
        x = x[None, :]
    if x.ndim != 2 or x.shape[0] == 0 or x.shape[1] == 0:
        raise HipError(E_INVALID, "clips must be a non-empty int16 [B, n] array")
    return x


def _size_query(entry, *ints):
    """A size entry of the C ABI (ints in, one size_t out) -> the bytes it answers."""
    lib = load_library()
    fn = getattr(lib, entry)
    fn.argtypes = [C.c_int] * len(ints) + [C.POINTER(C.c_size_t)]
    b = C.c_size_t(0)
    _check(lib, fn(*(int(v) for v in ints), C.byref(b)))
    return b.value


def loudness_sub_block(rate):
    """Samples of a 100 ms sub-block: Go's math.Round(0.1 rate) (audionorm/meter.go:91-93), not Python's round."""
    return int(math.floor(0.1 * float(rate) + 0.5))


def loudness_measure(clips_pcm16, rate, sub_energy=False, channels=1, device=0):
    """EBU R 128 integrated loudness and true peak of a batch of equally long mono clips in one device call (audionorm.MeasureInt16):
    int16 [B, n] (or [n]) at `rate` Hz -> list of B Loudness; with sub_energy also the float64 [B, n // S] K-weighted sub-block
    energies.  Spec: DESIGN.md §9."""
    lib = load_library()
    x = _mono_pcm16_clips("loudness", clips_pcm16, channels)
    out = (Loudness * x.shape[0])()
    sub = np.zeros((x.shape[0], x.shape[1] // max(1, loudness_sub_block(rate))), np.float64) if sub_energy else None
    lib.bnhip_loudness_measure_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    _check(lib, lib.bnhip_loudness_measure_pcm16(device, x.ctypes.data, x.shape[0], x.shape[1], int(rate), C.addressof(out),
                                                 sub.ctypes.data if sub is not None and sub.size else None))
    return (list(out), sub) if sub_energy else list(out)


def loudness_normalize(clips_pcm16, rate, target_lufs=-23.0, true_peak_dbtp=-1.0, max_gain_db=30.0, gate_fallback=False, apply=True,
                       channels=1, device=0):
    """Measure, plan and (apply) gain a batch of equally long mono clips in one device call: int16 [B, n] -> (list of B Loudness, int16
    [B, n] output or None for apply=False).  (max_gain_db 60, gate_fallback) is the export plan (actions_database.go:1392-1438),
    (30, no fallback) the BirdWeather upload's (encode_native.go:25-66)."""
    lib = load_library()
    x = _mono_pcm16_clips("loudness", clips_pcm16, channels)
    out = (Loudness * x.shape[0])()
    y = np.empty_like(x) if apply else None
    lib.bnhip_loudness_normalize_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                                   C.c_int, C.c_void_p, C.c_void_p]
    _check(lib, lib.bnhip_loudness_normalize_pcm16(device, x.ctypes.data, x.shape[0], x.shape[1], int(rate), float(target_lufs),
                                                   float(true_peak_dbtp), float(max_gain_db), 1 if gate_fallback else 0,
                                                   y.ctypes.data if apply else None, C.addressof(out)))
    return list(out), y


def loudness_workspace_size(n_clips, n, rate):
    """Bytes of device scratch loudness_normalize_device needs."""
    return _size_query("bnhip_loudness_workspace_size", n_clips, n, rate)


def loudness_normalize_device(d_pcm_ptr, n_clips, n, rate, d_out_ptr, d_workspace_ptr, workspace_bytes, d_out_pcm_ptr=None,
                              target_lufs=-23.0, true_peak_dbtp=-1.0, max_gain_db=30.0, gate_fallback=False, device=0, hip_stream_ptr=None):
    """Device-resident form: int16 clips, the Loudness results ([n_clips] of 80 bytes), the output clips and the workspace are device
    pointers; enqueued on the stream, not synchronised."""
    lib = load_library()
    lib.bnhip_loudness_normalize_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                                    C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    _check(lib, lib.bnhip_loudness_normalize_device(device, d_pcm_ptr, int(n_clips), int(n), int(rate), float(target_lufs),
                                                    float(true_peak_dbtp), float(max_gain_db), 1 if gate_fallback else 0, d_out_pcm_ptr,
                                                    d_out_ptr, d_workspace_ptr, int(workspace_bytes), hip_stream_ptr))


def denoise(clips_pcm16, frame, nr_db, nf_db, channels=1, device=0):
    """Spectral noise reduction of a batch of equally long mono clips in one device call (the afftdn stage of
    ffmpeg/process.go:212-251): int16 [B, n] (or [n]) -> int16 [B, n].  frame: a power of two in 64..4096; nr_db in [0, 97];
    nf_db in [-80, -20].  Spec: DESIGN.md §9 "Denoise"."""
    lib = load_library()
    x = _mono_pcm16_clips("denoise", clips_pcm16, channels)
    y = np.empty_like(x)
    lib.bnhip_denoise_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p]
    _check(lib, lib.bnhip_denoise_pcm16(device, x.ctypes.data, x.shape[0], x.shape[1], int(frame), float(nr_db), float(nf_db), y.ctypes.data))
    return y


def denoise_workspace_size(n_clips, n, frame):
    """Bytes of device scratch denoise_device asks for."""
    return _size_query("bnhip_denoise_workspace_size", n_clips, n, frame)


def denoise_device(d_pcm_ptr, n_clips, n, frame, nr_db, nf_db, d_out_pcm_ptr, d_workspace_ptr, workspace_bytes, device=0, hip_stream_ptr=None):
    """Device-resident form: the clips, the output clips (distinct) and the workspace are device pointers; enqueued on the stream,
    not synchronised."""
    lib = load_library()
    lib.bnhip_denoise_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                         C.c_size_t, C.c_void_p]
    _check(lib, lib.bnhip_denoise_device(device, d_pcm_ptr, int(n_clips), int(n), int(frame), float(nr_db), float(nf_db), d_out_pcm_ptr,
                                         d_workspace_ptr, int(workspace_bytes), hip_stream_ptr))


def process(clips_pcm16, rate, frame=0, nr_db=0.0, nf_db=-40.0, normalize=False, target_lufs=-23.0, true_peak_dbtp=-2.0, gain_db=0.0,
            channels=1, device=0):
    """The processed-audio chain denoise -> normalise -> gain (BuildProcessingFilterChain, ffmpeg/process.go:212-251) in one call,
    the clips staying on the device between the stages: int16 [B, n] -> (int16 [B, n], list of B Loudness or None without
    normalize).  frame 0: no denoise."""
    lib = load_library()
    x = _mono_pcm16_clips("process", clips_pcm16, channels)
    y = np.empty_like(x)
    res = (Loudness * x.shape[0])() if normalize else None
    lib.bnhip_process_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double,
                                        C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    _check(lib, lib.bnhip_process_pcm16(device, x.ctypes.data, x.shape[0], x.shape[1], int(rate), int(frame), float(nr_db), float(nf_db),
                                        1 if normalize else 0, float(target_lufs), float(true_peak_dbtp), float(gain_db), y.ctypes.data,
                                        C.addressof(res) if normalize else None))
    return y, (list(res) if normalize else None)


def flac_max_bytes(n_clips, n, seek_interval=0):
    """The worst-case bytes of n_clips streams of n samples (every frame VERBATIM): the out_cap the encode entries ask for."""
    return _size_query("bnhip_flac_max_bytes", n_clips, n, seek_interval)


def flac_workspace_size(n_clips, n):
    """Bytes of device scratch flac_encode_device needs."""
    return _size_query("bnhip_flac_workspace_size", n_clips, n)


def flac_lpc_workspace_size(n_clips, n, lpc_order):
    """Bytes of device scratch flac_encode_device needs with that lpc_order (0: flac_workspace_size)."""
    return _size_query("bnhip_flac_lpc_workspace_size", n_clips, n, lpc_order)


def _flac_streams(buf, offsets):
    return [buf[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in range(len(offsets) - 1)]


def flac_encode(clips_pcm16, rate, factor=None, seek_interval=0, channels=1, device=0, raw=False, lpc_order=0):
    """FLAC streams of a batch of equally long mono clips in one device call (flac.EncodePCMToBuffer; with seek_interval = rate what
    flac.EncodePCM writes to a file): int16 [B, n] (or [n]) -> list of B bytes objects.  factor: per-clip gain applied on the device
    first (None = none).  raw: (the uint8 buffer as written, offsets uint64 [B + 1]) instead.  lpc_order: 0, or M in 1..8 to try
    LPC subframes of orders 1..M as well (flac.LEVEL5_LPC_ORDER for the reference's level).  Spec: DESIGN.md §9."""
    lib = load_library()
    x = _mono_pcm16_clips("FLAC", clips_pcm16, channels)
    B, n = x.shape
    fac = None if factor is None else np.ascontiguousarray(factor, np.float64).reshape(-1)
    if fac is not None and fac.size != B:
        raise HipError(E_INVALID, f"factor must hold one value per clip, got {fac.size} for {B}")
    cap = flac_max_bytes(B, n, seek_interval)
    out = np.empty(cap, np.uint8)
    offsets = np.zeros(B + 1, np.uint64)
    lib.bnhip_flac_lpc_encode_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                                C.c_void_p, C.c_int]
    _check(lib, lib.bnhip_flac_lpc_encode_pcm16(device, x.ctypes.data, B, n, int(rate), fac.ctypes.data if fac is not None else None,
                                                int(seek_interval), out.ctypes.data, cap, offsets.ctypes.data, int(lpc_order)))
    return (out[:int(offsets[B])], offsets) if raw else _flac_streams(out, offsets)


def flac_encode_device(d_pcm_ptr, n_clips, n, rate, d_out_ptr, out_cap, d_offsets_ptr, d_workspace_ptr, workspace_bytes, d_factor_ptr=None,
                       seek_interval=0, device=0, hip_stream_ptr=None, lpc_order=0):
    """Device-resident form: the clips, the factors (nullable), the output, the uint64 [n_clips + 1] offsets and the workspace
    (flac_lpc_workspace_size of the same lpc_order) are device pointers; enqueued on the stream, not synchronised."""
    lib = load_library()
    lib.bnhip_flac_lpc_encode_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                                 C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
    _check(lib, lib.bnhip_flac_lpc_encode_device(device, d_pcm_ptr, int(n_clips), int(n), int(rate), d_factor_ptr, int(seek_interval),
                                                 d_out_ptr, int(out_cap), d_offsets_ptr, d_workspace_ptr, int(workspace_bytes), hip_stream_ptr,
                                                 int(lpc_order)))


def loudness_flac(clips_pcm16, rate, target_lufs=-23.0, true_peak_dbtp=-1.0, max_gain_db=30.0, gate_fallback=False, seek_interval=0,
                  channels=1, device=0, lpc_order=0):
    """loudness_normalize and flac_encode in one device call - the normalised clips never reach the host: int16 [B, n] -> (list of B
    Loudness, list of B bytes objects).  The BirdWeather upload is (30, no fallback, no seek table), a saved detection (60,
    fallback, seek_interval = rate).  lpc_order as flac_encode's."""
    lib = load_library()
    x = _mono_pcm16_clips("FLAC", clips_pcm16, channels)
    B, n = x.shape
    res = (Loudness * B)()
    cap = flac_max_bytes(B, n, seek_interval)
    out = np.empty(cap, np.uint8)
    offsets = np.zeros(B + 1, np.uint64)
    lib.bnhip_loudness_flac_lpc_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int,
                                                  C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
    _check(lib, lib.bnhip_loudness_flac_lpc_pcm16(device, x.ctypes.data, B, n, int(rate), float(target_lufs), float(true_peak_dbtp),
                                                  float(max_gain_db), 1 if gate_fallback else 0, int(seek_interval), C.addressof(res),
                                                  out.ctypes.data, cap, offsets.ctypes.data, int(lpc_order)))
    return list(res), _flac_streams(out, offsets)


def ragged_pack(clips):
    """A ragged burst as the bnhip_*_ragged_* entries take it: a list of 1-D int16 clips of any lengths >= 1 -> (the samples packed back
    to back, int16 [sum of lengths]; the lengths, int32 [n_clips]).  Anything but mono int16 is BNHIP_E_UNSUPPORTED, an empty burst or
    an empty clip BNHIP_E_INVALID."""
    clips = [np.ascontiguousarray(c) for c in clips]
    for c in clips:
        if c.dtype != np.int16 or c.ndim != 1:
            raise HipError(E_UNSUPPORTED, "ragged entries take mono int16 clips")
    if not clips or any(c.size == 0 for c in clips):
        raise HipError(E_INVALID, "a ragged burst is a non-empty list of non-empty clips")
    return np.concatenate(clips), np.array([c.size for c in clips], np.int32)


def ragged_unpack(packed, lens):
    """The clips of a packed buffer, in order (copies)."""
    ends = np.cumsum(np.asarray(lens, np.int64))
    return [packed[int(e - n):int(e)].copy() for e, n in zip(ends, lens)]


def _ragged_lens(lens):
    x = np.ascontiguousarray(lens, np.int32).reshape(-1)
    if x.size == 0:
        raise HipError(E_INVALID, "a ragged burst holds at least one clip")
    return x


def _ragged_size_query(entry, lens, *ints):
    """A ragged size entry of the C ABI (n_clips, lens, ints in, one size_t out) -> the bytes it answers."""
    lib = load_library()
    x = _ragged_lens(lens)
    fn = getattr(lib, entry)
    fn.argtypes = [C.c_int, C.c_void_p] + [C.c_int] * len(ints) + [C.POINTER(C.c_size_t)]
    b = C.c_size_t(0)
    _check(lib, fn(x.size, x.ctypes.data, *(int(v) for v in ints), C.byref(b)))
    return b.value


def loudness_ragged_workspace_size(lens, rate):
    """Bytes of device scratch loudness_normalize_ragged_device needs for clips of these lengths."""
    return _ragged_size_query("bnhip_loudness_ragged_workspace_size", lens, rate)


def flac_ragged_max_bytes(lens, seek_interval=0):
    """The worst-case bytes of the streams of clips of these lengths: the sum of flac_max_bytes(1, n, seek_interval)."""
    return _ragged_size_query("bnhip_flac_ragged_max_bytes", lens, seek_interval)


def flac_ragged_workspace_size(lens, lpc_order=0):
    """Bytes of device scratch flac_encode_ragged_device needs for clips of these lengths."""
    return _ragged_size_query("bnhip_flac_ragged_workspace_size", lens, lpc_order)


def loudness_normalize_ragged(clips, rate, target_lufs=-23.0, true_peak_dbtp=-1.0, max_gain_db=30.0, gate_fallback=False, apply=True,
                              device=0):
    """loudness_normalize of a ragged burst in one device call: a list of 1-D int16 clips of any lengths -> (list of Loudness, list of
    int16 outputs or None for apply=False), both in the input's order.  apply=False is also the measurement."""
    lib = load_library()
    x, lens = ragged_pack(clips)
    out = (Loudness * lens.size)()
    y = np.empty_like(x) if apply else None
    lib.bnhip_loudness_ragged_normalize_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double,
                                                          C.c_int, C.c_void_p, C.c_void_p]
    _check(lib, lib.bnhip_loudness_ragged_normalize_pcm16(device, x.ctypes.data, lens.size, lens.ctypes.data, int(rate), float(target_lufs),
                                                          float(true_peak_dbtp), float(max_gain_db), 1 if gate_fallback else 0,
                                                          y.ctypes.data if apply else None, C.addressof(out)))
    return list(out), (ragged_unpack(y, lens) if apply else None)


def loudness_normalize_ragged_device(d_pcm_ptr, lens, rate, d_out_ptr, d_workspace_ptr, workspace_bytes, d_out_pcm_ptr=None, target_lufs=-23.0,
                                     true_peak_dbtp=-1.0, max_gain_db=30.0, gate_fallback=False, device=0, hip_stream_ptr=None):
    """Device-resident form: the packed clips, the Loudness results, the packed output clips and the workspace are device pointers,
    lens a host array; enqueued on the stream, not synchronised."""
    lib = load_library()
    x = _ragged_lens(lens)
    lib.bnhip_loudness_ragged_normalize_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double,
                                                           C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    _check(lib, lib.bnhip_loudness_ragged_normalize_device(device, d_pcm_ptr, x.size, x.ctypes.data, int(rate), float(target_lufs),
                                                           float(true_peak_dbtp), float(max_gain_db), 1 if gate_fallback else 0, d_out_pcm_ptr,
                                                           d_out_ptr, d_workspace_ptr, int(workspace_bytes), hip_stream_ptr))


def _ragged_factor(factor, n_clips):
    fac = None if factor is None else np.ascontiguousarray(factor, np.float64).reshape(-1)
    if fac is not None and fac.size != n_clips:
        raise HipError(E_INVALID, f"factor must hold one value per clip, got {fac.size} for {n_clips}")
    return fac


def flac_encode_ragged(clips, rate, factor=None, seek_interval=0, device=0, raw=False, lpc_order=0):
    """flac_encode of a ragged burst in one device call: a list of 1-D int16 clips of any lengths -> list of bytes objects in the
    input's order (raw: the uint8 buffer as written and offsets uint64 [n_clips + 1])."""
    lib = load_library()
    x, lens = ragged_pack(clips)
    B = int(lens.size)
    fac = _ragged_factor(factor, B)
    cap = flac_ragged_max_bytes(lens, seek_interval)
    out = np.empty(cap, np.uint8)
    offsets = np.zeros(B + 1, np.uint64)
    lib.bnhip_flac_ragged_encode_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
                                                   C.c_void_p, C.c_int]
    _check(lib, lib.bnhip_flac_ragged_encode_pcm16(device, x.ctypes.data, B, lens.ctypes.data, int(rate),
                                                   fac.ctypes.data if fac is not None else None, int(seek_interval), out.ctypes.data, cap,
                                                   offsets.ctypes.data, int(lpc_order)))
    return (out[:int(offsets[B])], offsets) if raw else _flac_streams(out, offsets)


def flac_encode_ragged_device(d_pcm_ptr, lens, rate, d_out_ptr, out_cap, d_offsets_ptr, d_workspace_ptr, workspace_bytes, d_factor_ptr=None,
                              seek_interval=0, device=0, hip_stream_ptr=None, lpc_order=0):
    """Device-resident form: the packed clips, the factors (nullable), the output, the uint64 [n_clips + 1] offsets and the workspace
    (flac_ragged_workspace_size of the same lengths and lpc_order) are device pointers, lens a host array; enqueued on the stream,
    not synchronised."""
    lib = load_library()
    x = _ragged_lens(lens)
    lib.bnhip_flac_ragged_encode_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                    C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
    _check(lib, lib.bnhip_flac_ragged_encode_device(device, d_pcm_ptr, x.size, x.ctypes.data, int(rate), d_factor_ptr, int(seek_interval),
                                                    d_out_ptr, int(out_cap), d_offsets_ptr, d_workspace_ptr, int(workspace_bytes),
                                                    hip_stream_ptr, int(lpc_order)))


def loudness_flac_ragged(clips, rate, target_lufs=-23.0, true_peak_dbtp=-1.0, max_gain_db=30.0, gate_fallback=False, seek_interval=0,
                         device=0, lpc_order=0):
    """loudness_flac of a ragged burst in one device call and one device allocation: a list of 1-D int16 clips of any lengths ->
    (list of Loudness, list of bytes objects), both in the input's order."""
    lib = load_library()
    x, lens = ragged_pack(clips)
    B = int(lens.size)
    res = (Loudness * B)()
    cap = flac_ragged_max_bytes(lens, seek_interval)
    out = np.empty(cap, np.uint8)
    offsets = np.zeros(B + 1, np.uint64)
    lib.bnhip_loudness_flac_ragged_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double,
                                                     C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
    _check(lib, lib.bnhip_loudness_flac_ragged_pcm16(device, x.ctypes.data, B, lens.ctypes.data, int(rate), float(target_lufs),
                                                     float(true_peak_dbtp), float(max_gain_db), 1 if gate_fallback else 0, int(seek_interval),
                                                     C.addressof(res), out.ctypes.data, cap, offsets.ctypes.data, int(lpc_order)))
    return list(res), _flac_streams(out, offsets)


def png_max_bytes(n_images, width, height):
    """The worst-case bytes of n_images PNG streams of width x height index images (every band stored): what out_cap must be at least."""
    return _size_query("bnhip_png_max_bytes", n_images, width, height)


def png_workspace_size(n_images, width, height):
    """Bytes of device scratch png_encode_device needs."""
    return _size_query("bnhip_png_workspace_size", n_images, width, height)


def _png_palette(palette):
    pal = np.ascontiguousarray(palette, np.uint8).reshape(-1)
    if pal.size != 768:
        raise HipError(E_INVALID, "palette must be a 256 x 3 uint8 table")
    return pal


def png_encode(images, palette, device=0, raw=False):
    """PNG streams of a batch of equally sized 8-bit index images in one device call (the file GenerateFromPCM,
    spectrogram/generator.go:425, gets from its sox child): uint8 [B, H, W] (or [H, W]) and a 256 x 3 palette -> list of B bytes
    objects, or with raw=True (the streams back to back as uint8, offsets uint64 [B + 1]).  Spec: DESIGN.md §9 "PNG"."""
    lib = load_library()
    x = np.ascontiguousarray(images, np.uint8)
    if x.ndim == 2:
        x = x[None]
    if x.ndim != 3 or x.size == 0:
        raise HipError(E_INVALID, "images must be a non-empty uint8 [B, H, W] array")
    pal = _png_palette(palette)
    B, h, w = x.shape
    cap = png_max_bytes(B, w, h)
    out, offsets = np.empty(cap, np.uint8), np.zeros(B + 1, np.uint64)
    lib.bnhip_png_encode_u8.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    _check(lib, lib.bnhip_png_encode_u8(device, x.ctypes.data, B, w, h, pal.ctypes.data, out.ctypes.data, cap, offsets.ctypes.data))
    return (out[:int(offsets[B])], offsets) if raw else _flac_streams(out, offsets)


def png_encode_device(d_images_ptr, n_images, width, height, palette, d_out_ptr, out_cap, d_offsets_ptr, d_workspace_ptr, workspace_bytes,
                      device=0, hip_stream_ptr=None):
    """Device-resident form: images, streams, offsets (uint64 [n_images + 1]) and workspace (png_workspace_size) are device pointers,
    the palette a host table; enqueued on the stream, not synchronised."""
    lib = load_library()
    pal = _png_palette(palette)
    lib.bnhip_png_encode_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                            C.c_void_p, C.c_size_t, C.c_void_p]
    _check(lib, lib.bnhip_png_encode_device(device, d_images_ptr, int(n_images), int(width), int(height), pal.ctypes.data, d_out_ptr,
                                            int(out_cap), d_offsets_ptr, d_workspace_ptr, int(workspace_bytes), hip_stream_ptr))


def spectrogram_png(clips_pcm16, rate, width, palette, rate_out=0, window=None, top_db=0.0, range_db=100.0, device=0, raw=False):
    """spectrogram and png_encode in one device call - the indices never reach the host: int16 [B, n] (or [n]) -> list of B PNG streams
    (raw=True: as png_encode), each decoding to the image `spectrogram` returns for the same arguments."""
    lib = load_library()
    x = np.ascontiguousarray(clips_pcm16, np.int16)
    if x.ndim == 1:
        x = x[None, :]
    if x.ndim != 2 or x.shape[0] == 0 or x.shape[1] == 0:
        raise HipError(E_INVALID, "clips must be a non-empty int16 [B, n] array")
    pal = _png_palette(palette)
    height, fft_size = spectrogram_size(width)
    keep, wp = _spectrogram_window(window, fft_size)
    B = x.shape[0]
    cap = png_max_bytes(B, width, height)
    out, offsets = np.empty(cap, np.uint8), np.zeros(B + 1, np.uint64)
    lib.bnhip_spectrogram_png_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    _check(lib, lib.bnhip_spectrogram_png_pcm16(device, x.ctypes.data, B, x.shape[1], int(rate), int(rate_out), int(width), height, wp,
                                                float(top_db), float(range_db), pal.ctypes.data, out.ctypes.data, cap, offsets.ctypes.data))
    del keep
    return (out[:int(offsets[B])], offsets) if raw else _flac_streams(out, offsets)


def spectrogram_ragged_workspace_size(lens, width):
    """Bytes of device scratch spectrogram_ragged_device needs for clips of these lengths at this width (one table row per clip)."""
    return _ragged_size_query("bnhip_spectrogram_ragged_workspace_size", lens, width, spectrogram_size(width)[0])


def spectrogram_ragged(clips, rate, width, rate_out=0, window=None, top_db=0.0, range_db=100.0, device=0):
    """spectrogram of a ragged burst in one device call: a list of 1-D int16 clips of any lengths -> uint8 [B, H, W], image i what
    `spectrogram` gives clip i alone."""
    lib = load_library()
    x, lens = ragged_pack(clips)
    height, fft_size = spectrogram_size(width)
    keep, wp = _spectrogram_window(window, fft_size)
    img = np.empty((lens.size, height, int(width)), np.uint8)
    lib.bnhip_spectrogram_ragged_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                                   C.c_double, C.c_double, C.c_void_p]
    _check(lib, lib.bnhip_spectrogram_ragged_pcm16(device, x.ctypes.data, lens.size, lens.ctypes.data, int(rate), int(rate_out), int(width),
                                                   height, wp, float(top_db), float(range_db), img.ctypes.data))
    del keep
    return img


def spectrogram_png_ragged(clips, rate, width, palette, rate_out=0, window=None, top_db=0.0, range_db=100.0, device=0, raw=False):
    """spectrogram_png of a ragged burst in one device call: a list of 1-D int16 clips of any lengths -> list of B PNG streams (raw=True:
    as png_encode), stream i decoding to image i of spectrogram_ragged."""
    lib = load_library()
    x, lens = ragged_pack(clips)
    pal = _png_palette(palette)
    height, fft_size = spectrogram_size(width)
    keep, wp = _spectrogram_window(window, fft_size)
    B = lens.size
    cap = png_max_bytes(B, width, height)
    out, offsets = np.empty(cap, np.uint8), np.zeros(B + 1, np.uint64)
    lib.bnhip_spectrogram_png_ragged_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                                       C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    _check(lib, lib.bnhip_spectrogram_png_ragged_pcm16(device, x.ctypes.data, B, lens.ctypes.data, int(rate), int(rate_out), int(width),
                                                       height, wp, float(top_db), float(range_db), pal.ctypes.data, out.ctypes.data, cap,
                                                       offsets.ctypes.data))
    del keep
    return (out[:int(offsets[B])], offsets) if raw else _flac_streams(out, offsets)


def spectrogram_ragged_device(d_samples_ptr, f32, lens, width, height, d_image_ptr, d_workspace_ptr, workspace_bytes, window=None, top_db=0.0,
                              range_db=100.0, device=0, hip_stream_ptr=None):
    """Device-resident form: the packed samples (int16, or float32 with f32, at the render rate), the uint8 [n_clips, height, width]
    image and the workspace (spectrogram_ragged_workspace_size) are device pointers, lens a host array; enqueued on the stream, not
    synchronised."""
    lib = load_library()
    x = _ragged_lens(lens)
    keep, wp = _spectrogram_window(window, 2 * (int(height) - 1))
    lib.bnhip_spectrogram_ragged_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double,
                                                    C.c_double, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    _check(lib, lib.bnhip_spectrogram_ragged_device(device, d_samples_ptr, 1 if f32 else 0, x.size, x.ctypes.data, int(width), int(height), wp,
                                                    float(top_db), float(range_db), d_image_ptr, d_workspace_ptr, int(workspace_bytes),
                                                    hip_stream_ptr))
    del keep


def denoise_ragged(clips, frame, nr_db, nf_db, device=0):
    """denoise of a ragged burst in one device call: a list of 1-D int16 clips of any lengths -> list of int16 outputs, clip i what
    `denoise` gives clip i alone, byte for byte."""
    lib = load_library()
    x, lens = ragged_pack(clips)
    y = np.empty_like(x)
    lib.bnhip_denoise_ragged_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p]
    _check(lib, lib.bnhip_denoise_ragged_pcm16(device, x.ctypes.data, lens.size, lens.ctypes.data, int(frame), float(nr_db), float(nf_db),
                                               y.ctypes.data))
    return ragged_unpack(y, lens)


def denoise_ragged_workspace_size(lens, frame):
    """Bytes of device scratch denoise_ragged_device needs for clips of these lengths: two prefix tables of len(lens) + 1 64-bit
    entries, rounded up to 256."""
    return _ragged_size_query("bnhip_denoise_ragged_workspace_size", lens, frame)


def denoise_ragged_device(d_pcm_ptr, lens, frame, nr_db, nf_db, d_out_pcm_ptr, d_workspace_ptr, workspace_bytes, device=0, hip_stream_ptr=None):
    """Device-resident form: the packed clips, the packed output clips (distinct) and the workspace are device pointers, lens a host
    array; enqueued on the stream, not synchronised."""
    lib = load_library()
    x = _ragged_lens(lens)
    lib.bnhip_denoise_ragged_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p,
                                                C.c_void_p, C.c_size_t, C.c_void_p]
    _check(lib, lib.bnhip_denoise_ragged_device(device, d_pcm_ptr, x.size, x.ctypes.data, int(frame), float(nr_db), float(nf_db), d_out_pcm_ptr,
                                                d_workspace_ptr, int(workspace_bytes), hip_stream_ptr))


def process_ragged(clips, rate, frame=0, nr_db=0.0, nf_db=-40.0, normalize=False, target_lufs=-23.0, true_peak_dbtp=-2.0, gain_db=0.0,
                   device=0):
    """`process` of a ragged burst in one device call: a list of 1-D int16 clips of any lengths -> (list of int16 outputs, list of
    Loudness or None without normalize), both in the input's order."""
    lib = load_library()
    x, lens = ragged_pack(clips)
    y = np.empty_like(x)
    res = (Loudness * lens.size)() if normalize else None
    lib.bnhip_process_ragged_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                               C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    _check(lib, lib.bnhip_process_ragged_pcm16(device, x.ctypes.data, lens.size, lens.ctypes.data, int(rate), int(frame), float(nr_db),
                                               float(nf_db), 1 if normalize else 0, float(target_lufs), float(true_peak_dbtp), float(gain_db),
                                               y.ctypes.data, C.addressof(res) if normalize else None))
    return ragged_unpack(y, lens), (list(res) if normalize else None)


def process_spectrogram_png_ragged(clips, rate, width, palette, frame=0, nr_db=0.0, nf_db=-40.0, normalize=False, target_lufs=-23.0,
                                   true_peak_dbtp=-2.0, gain_db=0.0, rate_out=0, window=None, top_db=0.0, range_db=100.0, want_pcm=False,
                                   device=0, raw=False):
    """process_ragged and spectrogram_png_ragged in one device call, the processed PCM staying on the device (ProcessedSpectrogramByID,
    media.go:1321): a list of 1-D int16 clips of any lengths -> (list of B PNG streams (raw=True: as png_encode), list of Loudness or
    None without normalize, list of the processed int16 clips or None without want_pcm)."""
    lib = load_library()
    x, lens = ragged_pack(clips)
    pal = _png_palette(palette)
    height, fft_size = spectrogram_size(width)
    keep, wp = _spectrogram_window(window, fft_size)
    B = lens.size
    cap = png_max_bytes(B, width, height)
    out, offsets = np.empty(cap, np.uint8), np.zeros(B + 1, np.uint64)
    res = (Loudness * B)() if normalize else None
    y = np.empty_like(x) if want_pcm else None
    lib.bnhip_process_spectrogram_png_ragged_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double,
                                                               C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int,
                                                               C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_size_t,
                                                               C.c_void_p, C.c_void_p, C.c_void_p]
    _check(lib, lib.bnhip_process_spectrogram_png_ragged_pcm16(device, x.ctypes.data, B, lens.ctypes.data, int(rate), int(frame), float(nr_db),
                                                               float(nf_db), 1 if normalize else 0, float(target_lufs), float(true_peak_dbtp),
                                                               float(gain_db), int(rate_out), int(width), height, wp, float(top_db),
                                                               float(range_db), pal.ctypes.data, out.ctypes.data, cap, offsets.ctypes.data,
                                                               C.addressof(res) if normalize else None, y.ctypes.data if want_pcm else None))
    del keep
    png = (out[:int(offsets[B])], offsets) if raw else _flac_streams(out, offsets)
    return png, (list(res) if normalize else None), (ragged_unpack(y, lens) if want_pcm else None)


FLAC_OK, FLAC_BAD_METADATA, FLAC_UNSUPPORTED, FLAC_CORRUPT = 0, 1, 2, 3


class FlacInfo(C.Structure):
    """bnhip_flac_info: one stream's STREAMINFO as bnhip_flac_stream_info reads it, and its verdict (status, a FLAC_* value)."""
    _fields_ = [("total_samples", C.c_uint64), ("audio_offset", C.c_uint64), ("rate", C.c_uint32), ("bits", C.c_uint32),
                ("channels", C.c_uint32), ("min_block", C.c_uint32), ("max_block", C.c_uint32), ("min_frame", C.c_uint32),
                ("max_frame", C.c_uint32), ("seek_points", C.c_uint32), ("status", C.c_int32), ("reserved", C.c_int32)]


class FlacDecodeResult(C.Structure):
    """bnhip_flac_decode_result: status (FLAC_*), the frames decoded, and where the chain of frames broke (0 on success)."""
    _fields_ = [("status", C.c_int32), ("frames", C.c_int32), ("fail_offset", C.c_uint64)]


def _flac_burst(streams):
    """A list of bytes-like FLAC streams -> (uint8 buffer of them back to back, offsets uint64 [n + 1])."""
    parts = [np.frombuffer(bytes(s), np.uint8) for s in streams]
    if not parts:
        raise HipError(E_INVALID, "a burst holds at least one stream")
    offsets = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    buf = np.concatenate(parts) if int(offsets[-1]) else np.zeros(0, np.uint8)
    return np.ascontiguousarray(np.concatenate([buf, np.zeros(1, np.uint8)])), offsets      # (a spare byte: never an empty buffer)


def flac_stream_info(stream):
    """The marker and metadata blocks of one FLAC stream, read on the host (no device) -> FlacInfo."""
    lib = load_library()
    buf = np.frombuffer(bytes(stream) + b"\0", np.uint8)
    info = FlacInfo()
    lib.bnhip_flac_stream_info.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    _check(lib, lib.bnhip_flac_stream_info(buf.ctypes.data, buf.size - 1, C.addressof(info)))
    return info


def flac_recording_info(stream):
    """bnhip_flac_recording_info: flac_stream_info with the acceptance of the recording entries (1 or 2 channels, 16 or 24 bits)."""
    lib = load_library()
    buf = np.frombuffer(bytes(stream) + b"\0", np.uint8)
    info = FlacInfo()
    lib.bnhip_flac_recording_info.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    _check(lib, lib.bnhip_flac_recording_info(buf.ctypes.data, buf.size - 1, C.addressof(info)))
    return info


def flac_decode_recordings(streams, device=0, guard=0):
    """bnhip_flac_decode_recordings: a burst of FLAC recordings (1 or 2 channels, 16 or 24 bits) decoded in one device call
    -> (pcm uint8: the recordings' interleaved PCM at their own depths, back to back; pcm_offsets uint64 [n + 1]; list of
    FlacDecodeResult).  guard: that many bytes of 0xA5 are kept in front of and behind the output and checked after the call."""
    lib = load_library()
    buf, offsets = _flac_burst(streams)
    n = len(streams)
    infos = [flac_recording_info(s) for s in streams]
    total = sum(int(i.total_samples) * int(i.channels) * (int(i.bits) // 8) for i in infos if i.status == FLAC_OK)
    room = np.full(total + 2 * guard + 1, 0xA5, np.uint8)
    out = room[guard:guard + total]
    pcm_offsets = np.zeros(n + 1, np.uint64)
    res = (FlacDecodeResult * n)()
    lib.bnhip_flac_decode_recordings.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    _check(lib, lib.bnhip_flac_decode_recordings(device, buf.ctypes.data, n, offsets.ctypes.data, room.ctypes.data + guard, total,
                                                 pcm_offsets.ctypes.data, C.addressof(res)))
    if guard and not (np.all(room[:guard] == 0xA5) and np.all(room[guard + total:] == 0xA5)):
        raise HipError(E_RUNTIME, "bnhip_flac_decode_recordings wrote outside its output")
    return out, pcm_offsets, list(res)


def flac_decode_recordings_workspace_size(infos, offsets):
    """Bytes of device scratch flac_decode_recordings_device needs (infos: flac_recording_info's)."""
    lib = load_library()
    arr = (FlacInfo * len(infos))(*infos)
    off = np.ascontiguousarray(offsets, np.uint64)
    out = C.c_size_t(0)
    lib.bnhip_flac_decode_recordings_workspace_size.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    _check(lib, lib.bnhip_flac_decode_recordings_workspace_size(len(infos), C.addressof(arr), off.ctypes.data, C.byref(out)))
    return int(out.value)


def flac_decode_recordings_device(d_streams_ptr, offsets, infos, d_pcm_ptr, pcm_cap_bytes, d_result_ptr, d_workspace_ptr, workspace_bytes,
                                  device=0, hip_stream_ptr=None):
    """Device-resident form of flac_decode_recordings: the streams, the PCM bytes (cleared on the stream first), the FlacDecodeResult
    [n] records and the workspace are device pointers; enqueued on the stream, not synchronised."""
    lib = load_library()
    arr = (FlacInfo * len(infos))(*infos)
    off = np.ascontiguousarray(offsets, np.uint64)
    lib.bnhip_flac_decode_recordings_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                        C.c_void_p, C.c_size_t, C.c_void_p]
    _check(lib, lib.bnhip_flac_decode_recordings_device(device, d_streams_ptr, len(infos), off.ctypes.data, C.addressof(arr), d_pcm_ptr,
                                                        int(pcm_cap_bytes), d_result_ptr, d_workspace_ptr, int(workspace_bytes), hip_stream_ptr))


def flac_decode_workspace_size(infos, offsets):
    """Bytes of device scratch flac_decode_device needs for streams with these infos (a sequence of FlacInfo) and offsets."""
    lib = load_library()
    arr = (FlacInfo * len(infos))(*infos)
    off = np.ascontiguousarray(offsets, np.uint64)
    out = C.c_size_t(0)
    lib.bnhip_flac_decode_workspace_size.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    _check(lib, lib.bnhip_flac_decode_workspace_size(len(infos), C.addressof(arr), off.ctypes.data, C.byref(out)))
    return int(out.value)


def flac_decode_device(d_streams_ptr, offsets, infos, d_pcm_ptr, pcm_cap_samples, d_result_ptr, d_workspace_ptr, workspace_bytes, device=0,
                       hip_stream_ptr=None):
    """Device-resident form: the streams, the int16 clips, the FlacDecodeResult [n] records and the workspace
    (flac_decode_workspace_size) are device pointers, offsets and infos host arrays; enqueued on the stream, not synchronised."""
    lib = load_library()
    arr = (FlacInfo * len(infos))(*infos)
    off = np.ascontiguousarray(offsets, np.uint64)
    lib.bnhip_flac_decode_device.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                             C.c_void_p, C.c_size_t, C.c_void_p]
    _check(lib, lib.bnhip_flac_decode_device(device, d_streams_ptr, len(infos), off.ctypes.data, C.addressof(arr), d_pcm_ptr,
                                             int(pcm_cap_samples), d_result_ptr, d_workspace_ptr, int(workspace_bytes), hip_stream_ptr))


def flac_decode(streams, device=0):
    """A burst of FLAC streams (mono, 16 bits, fixed block size) decoded in one device call: a list of bytes objects -> (list of int16
    arrays, the clip of a stream whose metadata is not accepted being empty; list of FlacDecodeResult).  The samples of a stream whose
    status is not FLAC_OK are unspecified."""
    lib = load_library()
    buf, offsets = _flac_burst(streams)
    n = len(streams)
    infos = [flac_stream_info(s) for s in streams]
    total = sum(int(i.total_samples) for i in infos if i.status == FLAC_OK and i.total_samples <= 0x7FFFFFFF)
    pcm = np.empty(max(total, 1), np.int16)
    lens = np.zeros(n, np.int32)
    res = (FlacDecodeResult * n)()
    lib.bnhip_flac_decode_pcm16.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    _check(lib, lib.bnhip_flac_decode_pcm16(device, buf.ctypes.data, n, offsets.ctypes.data, pcm.ctypes.data, total, lens.ctypes.data,
                                            C.addressof(res)))
    return ragged_unpack(pcm, lens), list(res)


def flac_spectrogram_png(streams, width, palette, rate_out=0, window=None, top_db=0.0, range_db=100.0, device=0):
    """flac_decode and spectrogram_png_ragged in one device call - the PCM never reaches the host: a list of FLAC streams of one sample
    rate, every one with accepted metadata -> (list of PNG streams, list of FlacDecodeResult)."""
    lib = load_library()
    buf, offsets = _flac_burst(streams)
    n = len(streams)
    pal = _png_palette(palette)
    height, fft_size = spectrogram_size(width)
    keep, wp = _spectrogram_window(window, fft_size)
    cap = png_max_bytes(n, width, height)
    out, png_offsets = np.empty(cap, np.uint8), np.zeros(n + 1, np.uint64)
    res = (FlacDecodeResult * n)()
    lib.bnhip_flac_spectrogram_png.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double,
                                               C.c_double, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    _check(lib, lib.bnhip_flac_spectrogram_png(device, buf.ctypes.data, n, offsets.ctypes.data, int(rate_out), int(width), height, wp,
                                               float(top_db), float(range_db), pal.ctypes.data, out.ctypes.data, cap, png_offsets.ctypes.data,
                                               C.addressof(res)))
    del keep
    return _flac_streams(out, png_offsets), list(res)


def _sigmoid_f32div(x):
    """onnx/postprocess.go:8-10: 1.0 / (1.0 + float32(exp(float64(-x)))), the division in float32."""
    x = np.asarray(x, np.float32)
    e = np.exp(-x.astype(np.float64)).astype(np.float32)
    return (np.float32(1.0) / (np.float32(1.0) + e)).astype(np.float32)


class CustomClassifier:
    """inference.CustomClassifier (backend.go:31-52): secondary head on embedding vectors, e.g. a BattyBirdNET
    regional classifier.  PredictEmbedding returns sigmoid-applied scores (custom_classifier.go:148-174)."""

    def __init__(self, head_bytes: bytes, labels, device=0, max_batch=256):
        self._clf = HipClassifier(head_bytes, device=device, max_batch=max_batch)
        if len(labels) != self._clf.num_species():
            raise HipError(E_INVALID, f"label count {len(labels)} != head outputs {self._clf.num_species()}")
        self._labels = list(labels)

    def predict_embedding(self, embeddings):
        e = np.ascontiguousarray(embeddings, np.float32).reshape(-1)
        if e.size != self.input_dim():
            raise HipError(E_INVALID, f"input size mismatch: expected {self.input_dim()} values, got {e.size}")
        return _sigmoid_f32div(self._clf.predict_batch(e, 1)[0])

    def predict_embedding_batch(self, embeddings, batch_size):
        return _sigmoid_f32div(self._clf.predict_batch(embeddings, batch_size))

    def num_classes(self):
        return self._clf.num_species()

    def input_dim(self):
        return self._clf.n_samples

    def labels(self):
        return list(self._labels)

    def close(self):
        self._clf.close()


class RangeFilter:
    """inference.RangeFilter / BatchRangeFilter (backend.go:55-76): [lat, lon, week] -> per-species occurrence."""

    def __init__(self, model_bytes: bytes, device=0, max_batch=1024):
        self._clf = HipClassifier(model_bytes, device=device, max_batch=max_batch)
        if self._clf.n_samples != 3:
            raise HipError(E_INVALID, f"range filter model must take 3 inputs, takes {self._clf.n_samples}")

    def predict(self, latitude, longitude, week):
        return self._clf.predict_batch(np.asarray([latitude, longitude, week], np.float32), 1)[0]

    def predict_batch(self, inputs, batch_size):
        x = np.ascontiguousarray(inputs, np.float32).reshape(-1)
        if x.size != batch_size * 3:
            raise HipError(E_INVALID, f"input size mismatch: expected {batch_size * 3} values, got {x.size}")
        return self._clf.predict_batch(x, batch_size).reshape(-1)

    def heatmap(self, coords, species, stride=1, total_weeks=48):
        """One species' occurrence over a grid (HeatmapInferenceService.ComputeGridWithBinding, heatmap_service.go:143-420):
        coords [n_cells, 2] lat / lon -> float32 [ceil(total_weeks / stride), n_cells], row wi for week 1 + wi * stride."""
        self._clf._alive()
        c = np.ascontiguousarray(coords, np.float32).reshape(-1)
        if c.size % 2:
            raise HipError(E_INVALID, f"coords must hold lat / lon pairs, got {c.size} values")
        n_cells = c.size // 2
        weeks = (total_weeks + stride - 1) // stride if stride > 0 and total_weeks > 0 else 0
        out = np.empty((max(weeks, 0), n_cells), np.float32)
        lib = self._clf._lib
        lib.bnhip_range_heatmap.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        rc = lib.bnhip_range_heatmap(self._clf._h, c.ctypes.data, n_cells, int(species), int(stride), int(total_weeks),
                                     out.ctypes.data)
        if rc < 0:
            _check(lib, rc)
        assert rc == weeks, (rc, weeks)
        return out

    def num_species(self):
        return self._clf.num_species()

    def close(self):
        self._clf.close()


def heatmap_grid(south, north, west, east, resolution):
    """heatmapGridDimensions and the cell centres of computeHeatmapGrid (internal/api/v2/analytics/heatmap.go:212-219,
    315-330): rows = max(1, ceil((north - south) / resolution)), the same for cols; cell (row, col) is
    float32(south + (row + 0.5) * resolution), float32(west + (col + 0.5) * resolution), computed in float64.
    -> (rows, cols, coords float32 [rows * cols, 2] in row-major cell order)."""
    rows = max(1, int(math.ceil((north - south) / resolution)))
    cols = max(1, int(math.ceil((east - west) / resolution)))
    lat = (south + (np.arange(rows, dtype=np.float64) + 0.5) * resolution).astype(np.float32)
    lon = (west + (np.arange(cols, dtype=np.float64) + 0.5) * resolution).astype(np.float32)
    coords = np.empty((rows * cols, 2), np.float32)
    coords[:, 0] = np.repeat(lat, cols)
    coords[:, 1] = np.tile(lon, rows)
    return rows, cols, coords


class Bat:
    """Bat.Predict (classifier/bat_onnx.go:220-342): v2.4 backbone -> 1024-d embedding -> regional head ->
    plain sigmoid -> confidence threshold -> top-10.  The audio is 256 kHz material fed as if 48 kHz."""

    TOP_K = 10

    def __init__(self, backbone: HipClassifier, head: CustomClassifier, threshold=0.0):
        if not backbone.emb_dim:
            raise HipError(E_INVALID, "backbone model exposes no embedding output")
        if head.input_dim() != backbone.emb_dim:
            raise HipError(E_INVALID, f"head expects {head.input_dim()}-d embeddings, backbone yields {backbone.emb_dim}")
        self.backbone, self.head, self.threshold = backbone, head, float(threshold)

    def predict(self, samples):
        _, emb = self.backbone.predict_with_embeddings(samples)
        scores = self.head.predict_embedding(emb)
        order = np.argsort(-scores, kind="stable")
        labels = self.head.labels()
        return [(labels[i], float(scores[i])) for i in order if scores[i] >= self.threshold][:self.TOP_K]


class Resampler:
    """Resampler (internal/audiocore/resample/resample.go:57-172) on the GPU, stateless per clip.
    `resample_to(pcm16)` keeps the reference's int16 edges; `resample_f32` is the float path."""

    def __init__(self, from_rate, to_rate, device=0):
        if from_rate <= 0 or to_rate <= 0:
            raise HipError(E_INVALID, f"failed to create resampler from {from_rate} Hz to {to_rate} Hz")
        self.from_rate, self.to_rate, self.device = int(from_rate), int(to_rate), device
        self._lib = load_library()
        self._lib.bnhip_resample_f32.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        self._lib.bnhip_resample_pcm16.argtypes = self._lib.bnhip_resample_f32.argtypes

    def estimate_output(self, n_in):
        return int(self._lib.bnhip_resample_length(int(n_in), self.from_rate, self.to_rate))

    def _run(self, fn, x, dtype):
        x = np.ascontiguousarray(x, dtype)
        flat = x.ndim == 1
        if flat:
            x = x[None, :]
        no = self.estimate_output(x.shape[1])
        out = np.empty((x.shape[0], no), dtype)
        n = C.c_int(0)
        _check(self._lib, fn(self.device, x.ctypes.data, x.shape[0], x.shape[1], self.from_rate, self.to_rate,
                             out.ctypes.data, no, C.byref(n)))
        return out[0] if flat else out

    def resample_f32(self, samples):
        return self._run(self._lib.bnhip_resample_f32, samples, np.float32)

    def resample_to(self, pcm16):
        """int16 in -> int16 out (ResampleTo); accepts raw little-endian bytes or an int16 array."""
        if isinstance(pcm16, (bytes, bytearray)):
            if len(pcm16) % 2:
                raise HipError(E_INVALID, f"input length {len(pcm16)} is not a multiple of 2 (16-bit PCM requires even byte count)")
            return self._run(self._lib.bnhip_resample_pcm16, np.frombuffer(pcm16, "<i2"), np.int16).tobytes()
        return self._run(self._lib.bnhip_resample_pcm16, pcm16, np.int16)


class StreamResampler:
    """The reference's stateful Resampler (internal/audiocore/resample/resample.go:44-224), method for method:
    NewResampler(from, to) returns None for equal rates; resample_to / resample_into consume 16-bit PCM frames of any size
    and return what the stream so far determines; the FIR history stays on the GPU between calls, so the concatenated
    output of any chunking equals one one-shot call over the whole stream, bit for bit (after `flush`)."""

    def __init__(self, from_rate, to_rate, device=0):
        self._lib = load_library()
        L = self._lib
        L.bnhip_resampler_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.bnhip_resampler_estimate.argtypes = [C.c_void_p, C.c_int]
        for fn in (L.bnhip_resampler_process_pcm16, L.bnhip_resampler_process_f32):
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        for fn in (L.bnhip_resampler_flush_pcm16, L.bnhip_resampler_flush_f32):
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.bnhip_resampler_destroy.argtypes = [C.c_void_p]
        self.from_rate, self.to_rate = int(from_rate), int(to_rate)
        self._h = C.c_void_p()
        _check(L, L.bnhip_resampler_create(device, self.from_rate, self.to_rate, C.byref(self._h)))

    @classmethod
    def new(cls, from_rate, to_rate, device=0):
        """NewResampler: None when no resampling is required (resample.go:58-60)."""
        return None if from_rate == to_rate else cls(from_rate, to_rate, device)

    def estimate_output_bytes(self, input_bytes):
        if input_bytes <= 0:
            return 0
        return int(self._lib.bnhip_resampler_estimate(self._h, input_bytes // 2)) * 2

    def resample_to(self, pcm: bytes, dst: bytearray):
        """ResampleTo(input, dst) -> bytes written; errors leave the stream state untouched."""
        self._alive()
        if len(pcm) == 0:
            return 0
        if len(pcm) % 2:
            raise HipError(E_INVALID, f"input length {len(pcm)} is not a multiple of 2 (16-bit PCM requires even byte count)")
        x = np.frombuffer(pcm, "<i2")
        buf = (C.c_char * len(dst)).from_buffer(dst)
        n = C.c_int(0)
        _check(self._lib, self._lib.bnhip_resampler_process_pcm16(self._h, x.ctypes.data, x.size, C.addressof(buf), len(dst) // 2, C.byref(n)))
        return n.value * 2

    def resample_into(self, pcm: bytes) -> bytes:
        dst = bytearray(self.estimate_output_bytes(len(pcm)))
        n = self.resample_to(pcm, dst)
        return bytes(dst[:n])

    def process_f32(self, samples):
        self._alive()
        x = np.ascontiguousarray(samples, np.float32).reshape(-1)
        out = np.empty(int(self._lib.bnhip_resampler_estimate(self._h, x.size)) if x.size else 0, np.float32)
        if not x.size:
            return out
        n = C.c_int(0)
        _check(self._lib, self._lib.bnhip_resampler_process_f32(self._h, x.ctypes.data, x.size, out.ctypes.data, out.size, C.byref(n)))
        return out[:n.value]

    def flush(self, pcm16=True, cap=1 << 16):
        """End of stream: the tail that needed future (zero) input; resets the state."""
        self._alive()
        out = np.empty(cap, np.int16 if pcm16 else np.float32)
        n = C.c_int(0)
        fn = self._lib.bnhip_resampler_flush_pcm16 if pcm16 else self._lib.bnhip_resampler_flush_f32
        _check(self._lib, fn(self._h, out.ctypes.data, out.size, C.byref(n)))
        return out[:n.value].tobytes() if pcm16 else out[:n.value]

    def close(self):
        if self._h:
            self._lib.bnhip_resampler_destroy(self._h)
            self._h = C.c_void_p()

    def _alive(self):
        if not self._h:
            raise HipError(E_INVALID, "resampler is closed")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _pcm16_frames(frames):
    """-> (int16 arrays kept alive, C array of their addresses, C array of their lengths) for the bank entries."""
    arrs = []
    for f in frames:
        if isinstance(f, (bytes, bytearray, memoryview)):
            if len(f) % 2:
                raise HipError(E_INVALID, f"input length {len(f)} is not a multiple of 2 (16-bit PCM requires even byte count)")
            arrs.append(np.frombuffer(f, "<i2"))
        else:
            arrs.append(np.ascontiguousarray(f, np.int16).reshape(-1))
    n = len(arrs)
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in arrs])
    lens = (C.c_int * max(n, 1))(*[a.size for a in arrs])
    return arrs, ptrs, lens


def _c_ints(values):
    v = [int(x) for x in values]
    return (C.c_int * max(len(v), 1))(*v)


def _split_frames(out, counts):
    """Packed int16 outputs and the per-frame sample counts -> one bytes object per frame."""
    res, pos = [], 0
    for c in counts:
        res.append(out[pos:pos + c].tobytes())
        pos += int(c)
    return res


class _StreamBank:
    """What every bank shares: the handle `_h` of bnhip_<_prefix>_*, its stream slots and the lifetime.  A subclass binds its own
    entries with _bind (they override the shared ones' argtypes)."""

    _prefix = _what = None

    def _bind(self, **argtypes):
        """Loads the library and declares the shared entries plus the subclass's own (entry suffix -> argtypes)."""
        self._lib = L = load_library()
        vp, ci = C.c_void_p, C.c_int
        types = dict(add_stream=[vp, C.POINTER(ci)], remove_stream=[vp, ci], destroy=[vp])
        types.update(argtypes)
        for name, t in types.items():
            getattr(L, f"bnhip_{self._prefix}_{name}").argtypes = t
        getattr(L, f"bnhip_{self._prefix}_destroy").restype = None
        self._h = C.c_void_p()
        return L

    def _fn(self, name):
        return getattr(self._lib, f"bnhip_{self._prefix}_{name}")

    def add_stream(self):
        s = C.c_int(-1)
        _check(self._lib, self._fn("add_stream")(self._alive(), C.byref(s)))
        return s.value

    def remove_stream(self, stream):
        _check(self._lib, self._fn("remove_stream")(self._alive(), int(stream)))

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p()

    def _alive(self):
        if not self._h:
            raise HipError(E_INVALID, f"{self._what} is closed")
        return self._h

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _PcmBank(_StreamBank):
    """What ResamplerBank and EqualizerBank share beyond that: `process` (one bytes object per frame) and `write_windows` (one
    ring write per frame, through _write).  A subclass bounds process's default out_cap with _out_bound."""

    _write = None

    def _bind(self, **argtypes):
        vp, ci = C.c_void_p, C.c_int
        L = super()._bind(**dict(dict(process_pcm16=[vp, ci, vp, vp, vp, vp, C.c_size_t, vp]), **argtypes))
        getattr(L, self._write).argtypes = [vp, vp, ci, vp, vp, vp, vp]
        return L

    def process(self, items, out_cap=None):
        """[(stream, pcm16 bytes | int16 array), ...] -> [bytes, ...] per frame.  out_cap (samples) defaults to the most the frames
        can give; a smaller one is the library's E_INVALID (for tests of that path)."""
        streams = _c_ints(s for s, _ in items)
        arrs, ptrs, lens = _pcm16_frames([f for _, f in items])
        if out_cap is None:
            out_cap = self._out_bound(arrs)
        out = np.empty(max(out_cap, 1), np.int16)
        counts = np.zeros(max(len(items), 1), np.int32)
        _check(self._lib, self._fn("process_pcm16")(self._alive(), len(items), streams, ptrs, lens, out.ctypes.data, out_cap,
                                                    counts.ctypes.data))
        return _split_frames(out, counts[:len(items)])

    def write_windows(self, win, items):
        """[(stream, source, pcm16), ...] -> each frame's result written into source `source` of win (stream.NativeWindows), one
        ring write per frame, without the samples leaving the library."""
        streams = _c_ints(s for s, _, _ in items)
        sources = _c_ints(src for _, src, _ in items)
        arrs, ptrs, lens = _pcm16_frames([f for _, _, f in items])
        win._check(getattr(self._lib, self._write)(win._alive(), self._alive(), len(items), streams, sources, ptrs, lens))


class ResamplerBank(_PcmBank):
    """`bnhip_resampler_bank` (include/bnhip.h): one StreamResampler per stream for many streams of one (from, to) rate pair,
    every call one device call.  `process([(stream, pcm16), ...])` -> one bytes object per frame, each what that stream's own
    StreamResampler returns for the frame in sequence (a stream may appear several times; its frames go in list order);
    `write_windows(win, [(stream, source, pcm16), ...])` writes each frame's result into `source` of a stream.NativeWindows,
    one ring write per frame (bnhip_windows_write_resampled).  Errors leave every stream untouched."""

    _prefix, _what, _write = "resampler_bank", "resampler bank", "bnhip_windows_write_resampled"

    def __init__(self, from_rate, to_rate, max_streams=256, device=0):
        vp, ci = C.c_void_p, C.c_int
        L = self._bind(create=[ci, ci, ci, ci, C.POINTER(vp)], estimate=[vp, ci], flush_pcm16=[vp, ci, vp, vp, C.c_size_t, vp])
        self.from_rate, self.to_rate, self.max_streams = int(from_rate), int(to_rate), int(max_streams)
        _check(L, L.bnhip_resampler_bank_create(device, self.from_rate, self.to_rate, self.max_streams, C.byref(self._h)))
        if not self._h:
            raise HipError(E_INVALID, "equal rates need no resampler bank (ResamplerBank.new returns None)")

    @classmethod
    def new(cls, from_rate, to_rate, max_streams=256, device=0):
        """None when no resampling is required, as NewResampler (resample.go:58-60)."""
        return None if from_rate == to_rate else cls(from_rate, to_rate, max_streams, device)

    def estimate_output_bytes(self, input_bytes):
        return int(self._lib.bnhip_resampler_bank_estimate(self._alive(), int(input_bytes) // 2)) * 2

    def _out_bound(self, arrs):                     # the sum of the frames' estimates
        return sum(int(self._lib.bnhip_resampler_bank_estimate(self._alive(), a.size)) for a in arrs)

    def flush(self, streams, cap=1 << 16):
        """End of each listed stream: the tail per stream; each then starts anew."""
        streams = list(streams)
        out = np.empty(cap, np.int16)
        counts = np.zeros(max(len(streams), 1), np.int32)
        _check(self._lib, self._lib.bnhip_resampler_bank_flush_pcm16(self._alive(), len(streams), _c_ints(streams), out.ctypes.data, cap,
                                                                      counts.ctypes.data))
        return _split_frames(out, counts[:len(streams)])


# equalizer.go's filter names -> bnhip.h BNHIP_EQ_*
EQ_TYPES = {"LowPass": 0, "HighPass": 1, "AllPass": 2, "BandPass": 3, "BandReject": 4, "LowShelf": 5, "HighShelf": 6, "Peaking": 7}


def _eq_design_fn(lib):
    lib.bnhip_eq_design.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p]
    return lib.bnhip_eq_design


def design_filter(type, rate, frequency, q=0.0, width=0.0, gain=0.0, passes=1):
    """One RBJ biquad as equalizer.go's New<type> constructor builds it -> raw section (b0, b1, b2, a0, a1, a2) as a tuple of
    floats (bnhip_eq_design).  An unknown type or parameters the constructor refuses (or that give non-finite coefficients)
    raise HipError(E_INVALID)."""
    if type not in EQ_TYPES:
        raise HipError(E_INVALID, f"unknown filter type {type!r}")
    lib = load_library()
    out = np.zeros(6, np.float64)
    _check(lib, _eq_design_fn(lib)(EQ_TYPES[type], float(rate), float(frequency), float(q), float(width), float(gain), int(passes),
                                   out.ctypes.data))
    return tuple(float(v) for v in out)


def build_filter_chain(settings, rate):
    """equalizer.BuildFilterChain (equalizer/builder.go): settings is conf.EqualizerSettings as a dict ({"enabled": bool,
    "filters": [{"type", "frequency", "q", "width", "gain", "passes"}, ...]}) -> [(section6, passes), ...], or None when the
    equalizer is disabled, has no filters, or none of them could be built.  passes < 1 becomes 1; unknown types and filters
    that fail validation are skipped."""
    if not settings or not settings.get("enabled") or not settings.get("filters"):
        return None
    chain = []
    for f in settings["filters"]:
        passes = max(int(f.get("passes", 0)), 1)
        if f.get("type") not in EQ_TYPES:
            continue
        try:
            sec = design_filter(f["type"], rate, f.get("frequency", 0.0), q=f.get("q", 0.0), width=f.get("width", 0.0),
                                gain=f.get("gain", 0.0), passes=passes)
        except HipError as e:
            if e.code != E_INVALID:
                raise
            continue
        chain.append((sec, passes))
    return chain or None


def gain_linear(gain_db):
    """The route's gainLinear: math.Pow(10, gainDB/20) (audio_pipeline_service.go:1005)."""
    return 10.0 ** (float(gain_db) / 20.0)


class EqualizerBank(_PcmBank):
    """`bnhip_eq_bank` (include/bnhip.h): the analysis route's EQ chain + gain (AudioRouter.applyProcessing) for many streams,
    every call one device call.  `set_chain(stream, chain, gain_linear)` installs [(section6, passes), ...] (None or [] = no
    filters) with zero state; `process([(stream, pcm16), ...])` -> one bytes object per frame, as many samples as its input (a
    stream may appear several times; its frames go in list order); `write_windows(win, [(stream, source, pcm16), ...])` writes
    each frame's result into `source` of a stream.NativeWindows, one ring write per frame.  Errors leave every stream untouched."""

    MAX_STAGES = 16
    _prefix, _what, _write = "eq_bank", "equalizer bank", "bnhip_windows_write_equalized"

    def __init__(self, max_streams=256, device=0):
        vp, ci = C.c_void_p, C.c_int
        L = self._bind(create=[ci, ci, C.POINTER(vp)], set_chain=[vp, ci, vp, ci, vp, C.c_double], reset=[vp, ci])
        self.max_streams = int(max_streams)
        _check(L, L.bnhip_eq_bank_create(device, self.max_streams, C.byref(self._h)))

    def set_chain(self, stream, chain, gain_linear=1.0):
        chain = list(chain or [])
        secs = np.array([list(sec) for sec, _ in chain], np.float64).reshape(-1)
        passes = np.array([int(p) for _, p in chain], np.int32)
        _check(self._lib, self._lib.bnhip_eq_bank_set_chain(self._alive(), int(stream), secs.ctypes.data if chain else None, len(chain),
                                                            passes.ctypes.data if chain else None, float(gain_linear)))

    def reset(self, stream):
        _check(self._lib, self._lib.bnhip_eq_bank_reset(self._alive(), int(stream)))

    def _out_bound(self, arrs):                     # the total input
        return sum(a.size for a in arrs)


SOUNDLEVEL_MAX_BANDS = 32


class _SoundLevel(C.Structure):
    """bnhip_sound_level (include/bnhip.h): one SoundLevelData."""
    _fields_ = [("stream", C.c_int), ("frame", C.c_int), ("duration_s", C.c_int), ("n_bands", C.c_int),
                ("center_hz", C.c_double * 32), ("min_db", C.c_double * 32), ("max_db", C.c_double * 32),
                ("mean_db", C.c_double * 32), ("sample_count", C.c_int * 32)]


def sound_level_band_key(hz):
    """formatBandKey (soundlevel/processor.go:440-445): "%.1f_Hz" below 1 kHz, else "%.1f_kHz" of hz / 1000."""
    hz = float(hz)
    return "%.1f_Hz" % hz if hz < 1000 else "%.1f_kHz" % (hz / 1000)


def sound_level_bands(rate):
    """NewProcessor's 1/3-octave bands at `rate` (bnhip_soundlevel_bands) -> [(centre Hz, b0, b1, b2, a1, a2), ...] (normalised
    by a0).  rate <= 0 raises HipError(E_INVALID)."""
    lib = load_library()
    lib.bnhip_soundlevel_bands.argtypes = [C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    out = np.zeros((SOUNDLEVEL_MAX_BANDS, 6), np.float64)
    n = C.c_int(0)
    _check(lib, lib.bnhip_soundlevel_bands(int(rate), out.ctypes.data, SOUNDLEVEL_MAX_BANDS, C.byref(n)))
    return [tuple(float(v) for v in row) for row in out[:n.value]]


class SoundLevelBank(_StreamBank):
    """`bnhip_soundlevel_bank` (include/bnhip.h): one soundlevel.Processor per stream for many streams of one sample rate, every
    call one device call.  `add_stream(interval_s)` starts a fresh Processor; `process([(stream, pcm16), ...])` runs each frame
    as one ProcessSamples call (a stream may appear several times; its frames go in list order; an empty frame is not a call)
    and returns the finished reports in frame order, each {"stream", "frame", "duration_seconds", "octave_bands": {key:
    {"center_frequency_hz", "min_db", "max_db", "mean_db", "sample_count"}}}.  bands: None = NewProcessor's table for the rate,
    or [(centre, b0, b1, b2, a1, a2), ...] (as a Go host passes its own).  Errors leave every stream untouched."""

    _prefix, _what = "soundlevel_bank", "sound level bank"

    def __init__(self, sample_rate, max_streams=256, device=0, bands=None):
        vp, ci = C.c_void_p, C.c_int
        L = self._bind(create=[ci, ci, ci, vp, ci, C.POINTER(vp)], add_stream=[vp, ci, C.POINTER(ci)], reset=[vp, ci],
                       process_pcm16=[vp, ci, vp, vp, vp, vp, ci, C.POINTER(ci)])
        self.sample_rate, self.max_streams = int(sample_rate), int(max_streams)
        tbl = None if bands is None else np.ascontiguousarray(np.asarray(bands, np.float64).reshape(-1, 6))
        _check(L, L.bnhip_soundlevel_bank_create(device, self.sample_rate, self.max_streams, None if tbl is None else tbl.ctypes.data,
                                                 0 if tbl is None else len(tbl), C.byref(self._h)))

    def add_stream(self, interval_s=10):
        s = C.c_int(-1)
        _check(self._lib, self._lib.bnhip_soundlevel_bank_add_stream(self._alive(), int(interval_s), C.byref(s)))
        return s.value

    def reset(self, stream):
        _check(self._lib, self._lib.bnhip_soundlevel_bank_reset(self._alive(), int(stream)))

    def process(self, items, max_reports=None):
        """max_reports defaults to the non-empty frames (at most one report each); a smaller one can be the library's E_INVALID."""
        streams = _c_ints(s for s, _ in items)
        arrs, ptrs, lens = _pcm16_frames([f for _, f in items])
        if max_reports is None:
            max_reports = sum(1 for a in arrs if a.size)
        reps = (_SoundLevel * max(max_reports, 1))()
        n = C.c_int(0)
        _check(self._lib, self._lib.bnhip_soundlevel_bank_process_pcm16(self._alive(), len(items), streams, ptrs, lens, reps,
                                                                        int(max_reports), C.byref(n)))
        out = []
        for r in reps[:n.value]:
            bands = {}
            for j in range(r.n_bands):
                bands[sound_level_band_key(r.center_hz[j])] = {
                    "center_frequency_hz": r.center_hz[j], "min_db": r.min_db[j], "max_db": r.max_db[j], "mean_db": r.mean_db[j],
                    "sample_count": r.sample_count[j]}
            out.append({"stream": r.stream, "frame": r.frame, "duration_seconds": r.duration_s, "octave_bands": bands})
        return out


def audio_level(sum_squares, n, clipping):
    """bnhip_audio_level (host only): calculateAudioLevel's level 0..100 (buffer_consumer.go:310-331) from a frame's integers -
    the sum of the squares of its n int16 samples and whether any of them is full scale."""
    lib = load_library()
    lib.bnhip_audio_level.argtypes = [C.c_uint64, C.c_int64, C.c_int, C.POINTER(C.c_int)]
    level = C.c_int(0)
    _check(lib, lib.bnhip_audio_level(int(sum_squares), int(n), 1 if clipping else 0, C.byref(level)))
    return level.value


class LevelBank(_StreamBank):
    """`bnhip_level_bank` (include/bnhip.h, "Audio level bank"): the input level meter (calculateAudioLevel behind an
    AudioLevelConsumer route) for many sources of any rate, every call one device call.  `process([(stream, PCM), ...])` measures
    each frame (a stream may appear several times; an empty frame is a measurement) and returns the AUDIO_LEVEL records, one per
    frame: level 0..100, clipping, and the integers they came from.  `latest()` -> AUDIO_LEVEL [max_streams], stream -1 where dead or
    never measured; `stats(stream, reset)` -> the accumulators of AudioLevelStats and logAndReset's derived fields as a dict.
    Errors leave every stream untouched."""

    _prefix, _what = "level_bank", "level bank"

    def __init__(self, max_streams=256, device=0):
        vp, ci = C.c_void_p, C.c_int
        L = self._bind(create=[ci, ci, C.POINTER(vp)], process_pcm=[vp, ci, vp, vp, vp, ci, vp], latest=[vp, vp], stats=[vp, ci, ci, vp],
                       reset=[vp, ci])
        self.max_streams = int(max_streams)
        _check(L, L.bnhip_level_bank_create(device, self.max_streams, C.byref(self._h)))

    def process(self, frames, bit_depth=16):
        """A 16-bit frame of an odd byte count loses its last byte, as the reference truncates it; for 24 and 32 bit, bytes that are
        not whole samples are refused, as CaptureBank.write refuses them."""
        keep, n, ptr = _pcm_frames([f for _, f in frames], bit_depth, whole=False)
        st = np.array([int(s) for s, _ in frames], np.int32)
        out = np.zeros(max(len(keep), 1), AUDIO_LEVEL)
        _check(self._lib, self._lib.bnhip_level_bank_process_pcm(self._alive(), len(keep), st.ctypes.data, n.ctypes.data, ptr, int(bit_depth),
                                                                 out.ctypes.data))
        return out[:len(keep)]

    def latest(self):
        out = np.zeros(self.max_streams, AUDIO_LEVEL)
        _check(self._lib, self._lib.bnhip_level_bank_latest(self._alive(), out.ctypes.data))
        return out

    def stats(self, stream, reset=False):
        """reset: snapshot and start again, as logAndReset."""
        out = np.zeros(1, AUDIO_LEVEL_STATS)
        _check(self._lib, self._lib.bnhip_level_bank_stats(self._alive(), int(stream), 1 if reset else 0, out.ctypes.data))
        return {k: int(out[0][k]) for k in AUDIO_LEVEL_STATS.names if k != "_pad"}

    def reset(self, stream=-1):
        _check(self._lib, self._lib.bnhip_level_bank_reset(self._alive(), int(stream)))


class Perch:
    """Perch.Predict (classifier/perch_onnx.go:216-255): 160000 samples (32 kHz x 5 s) -> logits (graph output 3 of the
    reference's ONNX artefact, `:28`) -> perchSoftmax (`:315-335`: max-subtract, exp in float64, float32 running sum) ->
    label pairing -> top-10, with softmax + top-k on device.  `predict_with_embeddings` is the EmbeddingExtractor face
    (embedding = graph output 0, [1536])."""

    TOP_K = 10

    def __init__(self, classifier: HipClassifier, labels):
        if len(labels) != classifier.num_species():
            raise HipError(E_INVALID, f"label count {len(labels)} != model outputs {classifier.num_species()}")
        self.classifier, self.labels = classifier, list(labels)

    def predict(self, samples):
        conf, idx = self.classifier.predict_topk(np.asarray(samples, np.float32), 1, self.TOP_K, 1)
        return [(self.labels[i], float(c)) for c, i in zip(conf[0], idx[0])]

    def predict_batch(self, flat, batch_size):
        conf, idx = self.classifier.predict_topk(flat, batch_size, self.TOP_K, 1)
        return [[(self.labels[i], float(c)) for c, i in zip(cr, ir)] for cr, ir in zip(conf, idx)]

    def predict_with_embeddings(self, samples):
        return self.classifier.predict_with_embeddings(samples)


class BirdNET:
    """(*BirdNET).Predict (classifier/analyze.go:25-110): backend logits -> sigmoid(sensitivity) ->
    label pairing -> top-10, with the post-processing on device."""

    TOP_K = 10  # defaultTopKResults

    def __init__(self, classifier: HipClassifier, labels, sensitivity=1.0):
        if len(labels) != classifier.num_species():
            # validateModelAndLabels, classifier/birdnet.go:1248-1256
            raise HipError(E_INVALID, f"label count {len(labels)} != model outputs {classifier.num_species()}")
        self.classifier, self.labels, self.sensitivity = classifier, list(labels), float(sensitivity)

    def predict(self, samples):
        conf, idx = self.classifier.predict_topk(np.asarray(samples, np.float32), 1, self.TOP_K, 0, self.sensitivity)
        return [(self.labels[i], float(c)) for c, i in zip(conf[0], idx[0])]

    def predict_batch(self, flat, batch_size):
        conf, idx = self.classifier.predict_topk(flat, batch_size, self.TOP_K, 0, self.sensitivity)
        return [[(self.labels[i], float(c)) for c, i in zip(cr, ir)] for cr, ir in zip(conf, idx)]

    def predict_windows(self, win, bit_depth=16):
        """One tick for this model: every ready window of the assembler `win` (stream.NativeWindows) through one device call, the
        rows assembled under the device's work on the previous chunk (bnhip_windows_predict_topk).
        -> (source indices, uint8 rows view, per-window top-10 lists); a source index of -1 marks a row to skip."""
        idxs, rows, conf, idx = win.predict_topk(self.classifier, bit_depth, self.TOP_K, 0, self.sensitivity)
        return idxs, rows, [[(self.labels[i], float(c)) for c, i in zip(cr, ir)] for cr, ir in zip(conf, idx)]

    def predict_windows_events(self, win, bank, bit_depth=16):
        """predict_windows with the tick's rows also fed to `bank` (an EventBank on the model's device) in the same call
        (bnhip_windows_predict_events).  -> (source indices, rows view, per-window top-10 lists, the events that became due)."""
        idxs, rows, conf, idx, events = self.classifier.predict_windows_events(win, bank, bit_depth, self.TOP_K, 0, self.sensitivity)
        return idxs, rows, [[(self.labels[i], float(c)) for c, i in zip(cr, ir)] for cr, ir in zip(conf, idx)], events

    def predict_pcm_batch(self, raw, bit_depth, batch_size):
        """The windows' little-endian PCM bytes as captured (a1 runs in the kernel, process.go:479-497) -> per-window top-10."""
        conf, idx = self.classifier.predict_pcm_topk(raw, bit_depth, batch_size, self.TOP_K, 0, self.sensitivity)
        return [[(self.labels[i], float(c)) for c, i in zip(cr, ir)] for cr, ir in zip(conf, idx)]
