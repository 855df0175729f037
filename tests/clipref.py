"""numpy restatement of the detection-clip rules of include/bnhip.h ("Detection clips"): the span of an event, the float32 -> int16
rule of a cut sample, and the capacity rule of bnhip_analyze_channels_pcm_clips.  Integer arithmetic in Python ints; no device."""
import numpy as np

from birdnet_go_amd import host


def spans(events, resampled_length, hop, pre_samples, post_samples, max_samples, extended):
    """-> CLIP_SPAN [n_events]: begin = first_window * hop - pre, end = (extended ? last : first)_window * hop + post, both clamped to
    [0, N], then end = min(end, begin + max_samples); a status != 0 event gets length 0."""
    out = np.zeros(len(events), host.CLIP_SPAN)
    for i, e in enumerate(events):
        n = int(resampled_length[int(e["recording"])])
        begin = min(max(int(e["first_window"]) * hop - pre_samples, 0), n)
        end = min(max(int(e["last_window" if extended else "first_window"]) * hop + post_samples, 0), n)
        end = min(end, begin + max_samples)
        out[i] = (begin, 0 if int(e["status"]) != 0 else end - begin, int(e["recording"]))
    return out


def to_pcm16(x):
    """q = clamp(rint(x * 32768), -32768, 32767) of float32 samples: the product in float32 (exact, or an infinity), ties to even,
    a NaN gives 0."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.rint(x * np.float32(32768.0))
    y = np.where(np.isnan(y), np.float32(0.0), np.clip(y, np.float32(-32768.0), np.float32(32767.0)))
    return y.astype(np.int16)


def as_float32(raw, bits):
    """The float32 that the windows are framed from (csrc/pcm_sample.h), of the samples of one recording at depth `bits` (0: float32)."""
    if bits == 0:
        return np.frombuffer(raw, "<f4")
    if bits == 16:
        return np.frombuffer(raw, "<i2").astype(np.float32) / np.float32(32768.0)
    if bits == 32:
        return np.frombuffer(raw, "<i4").astype(np.float32) / np.float32(2147483648.0)
    b = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.int32)
    v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    v = np.where(v & 0x800000, v - (1 << 24), v)
    return v.astype(np.float32) / np.float32(8388608.0)


def cut(recordings_f32, span_table):
    """The clips of the spans of non-zero length, in span order, out of float32 recordings."""
    return [to_pcm16(recordings_f32[int(s["recording"])][int(s["start"]):int(s["start"]) + int(s["length"])])
            for s in span_table if int(s["length"]) > 0]


def capacity(span_table, flac_cap, seek_interval, png_cap=None, width=0, height=0):
    """n_clips: the largest n <= the spans of non-zero length, n <= 65535, with flac_ragged_max_bytes of the first n lengths <=
    flac_cap and, with width > 0, png_max_bytes(n, width, height) <= png_cap."""
    lens = [int(s["length"]) for s in span_table if int(s["length"]) > 0][:65535]
    n = 0
    while n < len(lens):
        if host.flac_ragged_max_bytes(lens[:n + 1], seek_interval) > flac_cap:
            break
        if width > 0 and host.png_max_bytes(n + 1, width, height) > png_cap:
            break
        n += 1
    return n
