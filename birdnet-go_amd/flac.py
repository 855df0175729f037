"""FLAC clip encoding: the surface of the reference's internal/audiocore/flac package that the BirdWeather upload and the detection
save see, over bnhip_flac_encode_pcm16 and bnhip_loudness_flac_pcm16.

  EncodePCMToBuffer                  flac/encode.go:320-369         -> encode_clips(.., seek_interval=0)
  EncodePCM (file, seek table)       flac/encode.go:79-175          -> encode_clips(.., seek_interval=sample_rate)
  encodeFLACNative                   birdweather/encode_native.go:28-98 -> normalize_and_encode(.., max_gain_db=DEFAULT_MAX_GAIN_DB)

  (reading a saved clip back)         spectrogram/generator.go:276-424 -> stream_info, decode_clips; spectrogram.generate_from_flac

Mono int16 only.  The bytes follow the project's own encoder spec: valid RFC 9639 streams, not go-flac's bytes.
lpc_order: 0 (the default) tries CONSTANT / FIXED / VERBATIM subframes only; M in 1..8 tries LPC orders 1..M as well.
"""
import numpy as np

from . import host as _host
from .loudness import DEFAULT_MAX_GAIN_DB, _burst, default_options, factor_from_db

# The reference encodes at go-flac's CompressionLevel 5 (flac/encode.go:25,136-145,350-358), an LPC level; this encoder's LPC search
# gains nothing above order 8 on the reference's own recording.
LEVEL5_LPC_ORDER = 8


def encode_clips(clips, sample_rate, gain_db=None, seek_interval=0, device=0, lpc_order=0, ragged=False):
    """A burst of detections: a list of int16 mono clips of any lengths -> list of FLAC streams (bytes) in the input's order.
    gain_db: None, one gain for all, or one per clip; applied on the device (FactorFromDB, then the saturating int16 gain).
    ragged: the whole burst in one device call (bnhip_flac_ragged_encode_pcm16) instead of one call per distinct length; the same
    bytes."""
    clips, groups = _burst(clips)
    if gain_db is None:
        factor = None
    else:
        g = np.broadcast_to(np.asarray(gain_db, np.float64), (len(clips),))
        factor = np.array([factor_from_db(float(v)) for v in g], np.float64)
    if ragged:
        return _host.flac_encode_ragged(clips, sample_rate, factor, seek_interval, device=device, lpc_order=lpc_order)
    streams = [None] * len(clips)
    for idx in groups.values():
        out = _host.flac_encode(np.stack([clips[i] for i in idx]), sample_rate, None if factor is None else factor[idx], seek_interval,
                                device=device, lpc_order=lpc_order)
        for j, i in enumerate(idx):
            streams[i] = out[j]
    return streams


def normalize_and_encode(clips, sample_rate, opts=None, max_gain_db=DEFAULT_MAX_GAIN_DB, gate_fallback=False, seek_interval=0, device=0,
                         lpc_order=0, ragged=False):
    """Loudness-normalise and encode a burst in one device call per length: -> (list of host.Loudness, list of FLAC streams), both
    in the input's order.  The normalised PCM never reaches the host.  ragged: the whole burst in one device call
    (bnhip_loudness_flac_ragged_pcm16), whatever its lengths."""
    opts = opts or default_options()
    clips, groups = _burst(clips)
    if ragged:
        return _host.loudness_flac_ragged(clips, sample_rate, opts.target_lufs, opts.true_peak_dbtp, max_gain_db, gate_fallback, seek_interval,
                                          device=device, lpc_order=lpc_order)
    results, streams = [None] * len(clips), [None] * len(clips)
    for idx in groups.values():
        res, out = _host.loudness_flac(np.stack([clips[i] for i in idx]), sample_rate, opts.target_lufs, opts.true_peak_dbtp, max_gain_db,
                                       gate_fallback, seek_interval, device=device, lpc_order=lpc_order)
        for j, i in enumerate(idx):
            results[i], streams[i] = res[j], out[j]
    return results, streams


def stream_info(stream):
    """The metadata of one FLAC stream, read on the host: -> host.FlacInfo (rate, bits, channels, total_samples, block and frame bounds,
    audio_offset, seek_points, and status: host.FLAC_OK, FLAC_BAD_METADATA or FLAC_UNSUPPORTED)."""
    return _host.flac_stream_info(stream)


def recording_info(stream):
    """stream_info with the acceptance of the recording decoder: 1 or 2 channels, 16 or 24 bits, a fixed block size up to 8192 (mono
    16-bit: 16384) -> host.FlacInfo."""
    return _host.flac_recording_info(stream)


def decode_recordings(streams, device=0, as_bytes=False):
    """Recordings read back: a list of FLAC streams of 1 or 2 channels at 16 or 24 bits -> (recordings, results) in the input's
    order, in one device call.  recordings[i] is an int16 (16-bit streams) or int32 (24-bit) array shaped [frames, channels] - or,
    with as_bytes, the interleaved little-endian PCM at the stream's own depth, exactly a WAV data chunk of the same audio -, and
    None where the stream's metadata is not accepted.  A stream whose results[i].status is host.FLAC_CORRUPT keeps the frames in
    front of the damage; every sample that was not restored is zero."""
    infos = [_host.flac_recording_info(s) for s in streams]
    pcm, offsets, results = _host.flac_decode_recordings(streams, device=device)
    out = []
    for i, info in enumerate(infos):
        if info.status != _host.FLAC_OK:
            out.append(None)
            continue
        b = pcm[int(offsets[i]):int(offsets[i + 1])]
        if as_bytes:
            out.append(b.tobytes())
        elif info.bits == 16:
            out.append(b.copy().view("<i2").reshape(-1, int(info.channels)))
        else:
            t = b.reshape(-1, 3).astype(np.int32)
            v = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)
            out.append((v - ((v & 0x800000) << 1)).astype(np.int32).reshape(-1, int(info.channels)))
    return out, results


def decode_clips(streams, device=0):
    """Saved clips read back: a list of FLAC streams (mono, 16 bits, fixed block size; what encode_clips writes and what a general
    encoder may write for mono int16) -> (clips, results) in the input's order, in one device call.  clips[i] is an int16 array, or
    None where results[i].status is not host.FLAC_OK; results[i] is a host.FlacDecodeResult (status, frames, fail_offset).  The
    STREAMINFO MD5 is not verified."""
    clips, results = _host.flac_decode(streams, device=device)
    return [c if r.status == _host.FLAC_OK else None for c, r in zip(clips, results)], results
