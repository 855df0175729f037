"""Detection-clip spectrogram images: the surface of the reference's internal/spectrogram package that a caller of
GenerateFromPCM (generator.go:425-530) sees, over bnhip_spectrogram_pcm16.

  SizeToPixels / PixelsToSize        utils.go:44-78            -> size_to_pixels / pixels_to_size
  fftFriendlyHeight                  generator.go:115-123      -> fft_friendly_height
  BirdProfile / BatProfile           frequency_profile.go      -> bird_profile / bat_profile
  style presets                      conf/config.go:252-255    -> palette(style), style_window(style, n)
  dynamic range presets              conf/config.go:262-264    -> DYNAMIC_RANGES
  GenerateFromPCM                    generator.go:425          -> generate_from_pcm, generate_batch (many clips, one device call),
                                                                  generate_burst (clips of any lengths)

Only raw images are produced (sox's -r: no axes, no legend), mono, as 8-bit indexed PNG.  The pixel values follow the project's own
rendering spec; they are not pinned against sox, which is not in the reference's tree.
"""
import os
import struct
import zlib
from dataclasses import dataclass

import numpy as np

from . import host as _host

SIZES = {"sm": 258, "md": 514, "lg": 1026, "xl": 2050}          # utils.go:50-55 (heights 129 / 257 / 513 / 1025)
STYLES = ("default", "scientific_dark", "high_contrast_dark", "scientific")      # conf/config.go:252-255
DYNAMIC_RANGES = ("80", "100", "120")                            # conf/config.go:262-264
DOLPH_EXTRA_DB = 20.0     # the "scientific" styles' Dolph window: side lobes at range_db + 20 dB below the main lobe (this project's choice)


def size_to_pixels(size):
    if size not in SIZES:
        raise ValueError(f'invalid spectrogram size "{size}" (valid sizes: sm, md, lg, xl)')
    return SIZES[size]


def pixels_to_size(width):
    for size, w in SIZES.items():
        if w == width:
            return size
    raise ValueError(f"invalid spectrogram width {width}: no matching size")


def fft_friendly_height(width):
    """The smallest 2^k + 1 that is >= width // 2, so that the transform length 2 (height - 1) is a power of two."""
    target = width // 2
    n = 1
    while n + 1 < target:
        n *= 2
    return n + 1


@dataclass(frozen=True)
class FrequencyProfile:
    resample_rate: int        # target rate in Hz; 0 keeps the native rate
    suffix: str = ""          # cache-file token of the profile ("" for the default bird render)


def bird_profile():
    return FrequencyProfile(24000)


def bat_profile():
    return FrequencyProfile(256000, "bat-v2")


def hann(n):
    """Periodic Hann, 0.5 - 0.5 cos(2 pi i / n): the window a NULL table means in the C ABI."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def dolph(n, atten_db):
    """Dolph-Chebyshev window of n points with every side lobe atten_db below the main lobe (sox's `-w dolph`), peak 1, symmetric.
    The textbook construction: sample the Chebyshev polynomial T_(n-1)(beta cos(pi k / n)), beta = cosh(acosh(10^(atten/20)) / (n-1)),
    and take its DFT."""
    n = int(n)
    if n < 2:
        return np.ones(max(n, 0))
    order = n - 1
    beta = np.cosh(np.arccosh(10.0 ** (abs(float(atten_db)) / 20.0)) / order)
    x = beta * np.cos(np.pi * np.arange(n) / n)
    p = np.zeros(n)
    hi, lo, mid = x > 1, x < -1, np.abs(x) <= 1
    p[hi] = np.cosh(order * np.arccosh(x[hi]))
    p[lo] = (2 * (n % 2) - 1) * np.cosh(order * np.arccosh(-x[lo]))
    p[mid] = np.cos(order * np.arccos(x[mid]))
    if n % 2:
        w = np.real(np.fft.fft(p))
        h = (n + 1) // 2
        w = np.concatenate((w[h - 1:0:-1], w[:h]))
    else:
        w = np.real(np.fft.fft(p * np.exp(1j * np.pi / n * np.arange(n))))
        h = n // 2 + 1
        w = np.concatenate((w[h - 1:0:-1], w[1:h]))
    return w / w.max()


def palette(style="default"):
    """256 x 3 uint8 colour table of a style preset; index 0 is the background, index 255 full intensity.  With t = i / 255 and
    clip(.) onto [0, 1], every channel is floor(255 c + 0.5):
      scientific_dark     grey ramp, c = t                                        (black background, white at full intensity)
      scientific          its inverse, c = 1 - t                                  (white background, black at full intensity)
      default             r = clip(2.4 t - 0.3), g = clip(2.4 t - 1.2), b = max(0.6 sin(2 pi t) for t < 0.5, clip(4 t - 3))
                          (black - violet - red - yellow - white)
      high_contrast_dark  r = clip(4 t - 1), g = clip(2 t - 1), b = max(clip(min(4 t, 2 - 4 t)), clip(4 t - 3))
                          (black - blue - red - yellow - white, steeper steps)
    These ramps are the project's own; sox's are not in the reference's tree."""
    t = np.arange(256) / 255.0
    clip = lambda v: np.clip(v, 0.0, 1.0)
    if style == "scientific_dark":
        r = g = b = t
    elif style == "scientific":
        r = g = b = 1.0 - t
    elif style == "default":
        r, g = clip(2.4 * t - 0.3), clip(2.4 * t - 1.2)
        b = np.maximum(np.where(t < 0.5, 0.6 * np.sin(2.0 * np.pi * t), 0.0), clip(4.0 * t - 3.0))
    elif style == "high_contrast_dark":
        r, g = clip(4.0 * t - 1.0), clip(2.0 * t - 1.0)
        b = np.maximum(clip(np.minimum(4.0 * t, 2.0 - 4.0 * t)), clip(4.0 * t - 3.0))
    else:
        raise ValueError(f'invalid spectrogram style "{style}" (valid styles: {", ".join(STYLES)})')
    return np.floor(255.0 * np.stack([r, g, b], axis=1) + 0.5).astype(np.uint8)


def style_window(style, n, range_db=100.0):
    """The window table of a style: Dolph for the two "scientific" styles (generator.go:149-157 `-w dolph`), None (periodic Hann) otherwise."""
    if style not in STYLES:
        raise ValueError(f'invalid spectrogram style "{style}" (valid styles: {", ".join(STYLES)})')
    return dolph(n, float(range_db) + DOLPH_EXTRA_DB) if style in ("scientific_dark", "scientific") else None


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(path, image, pal):
    """8-bit indexed PNG (colour type 3) of a uint8 [H, W] index image and a 256 x 3 palette; every scanline uses filter type 0."""
    img = np.ascontiguousarray(image, np.uint8)
    pal = np.ascontiguousarray(pal, np.uint8)
    if img.ndim != 2 or img.size == 0:
        raise ValueError("image must be a non-empty uint8 [H, W] array")
    if pal.shape != (256, 3):
        raise ValueError("palette must be a 256 x 3 uint8 table")
    h, w = img.shape
    rows = np.zeros((h, w + 1), np.uint8)
    rows[:, 1:] = img
    data = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 3, 0, 0, 0)) + _chunk(b"PLTE", pal.tobytes())
            + _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _chunk(b"IEND", b""))
    with open(path, "wb") as fh:
        fh.write(data)


def _render_args(sample_rate, width, profile, style, dynamic_range):
    if str(dynamic_range) not in DYNAMIC_RANGES:
        raise ValueError(f'invalid dynamic range "{dynamic_range}" (valid: 80, 100, 120)')
    if width <= 0:
        raise ValueError("width must be positive")
    if sample_rate <= 0:
        raise ValueError("sample rate must be positive")
    profile = profile or bird_profile()
    range_db = float(dynamic_range)
    _, fft_size = _host.spectrogram_size(width)
    return dict(rate_out=profile.resample_rate, window=style_window(style, fft_size, range_db), top_db=0.0, range_db=range_db)


def _render(clips, sample_rate, width, profile, style, dynamic_range, device):
    kw = _render_args(sample_rate, width, profile, style, dynamic_range)
    return _host.spectrogram(clips, sample_rate, width, device=device, **kw), palette(style)


def read_png_indices(data):
    """The uint8 [H, W] indices of one of the device encoder's streams (8-bit indexed, filter type 0 on every row; DESIGN.md §9 "PNG")."""
    pos, idat, shape = 8, [], None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if kind == b"IHDR":
            shape = struct.unpack(">II", body[:8])
        elif kind == b"IDAT":
            idat.append(body)
        pos += 12 + n
    w, h = shape
    rows = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(h, w + 1)
    if rows[:, 0].any():
        raise ValueError("a row's filter type is not 0")
    return rows[:, 1:].copy()


def _render_png(clips, output_paths, sample_rate, width, profile, style, dynamic_range, device):
    """Render and encode in one device call; the files are the device's streams, the indices come back out of them."""
    kw = _render_args(sample_rate, width, profile, style, dynamic_range)
    streams = _host.spectrogram_png(clips, sample_rate, width, palette(style), device=device, **kw)
    for p, s in zip(output_paths, streams):
        with open(p, "wb") as fh:
            fh.write(s)
    return np.stack([read_png_indices(s) for s in streams])


def generate_from_pcm(pcm_bytes, output_path, width, sample_rate, profile=None, style="default", dynamic_range="100", device=0,
                      device_png=False):
    """GenerateFromPCM (generator.go:425): 16-bit little-endian mono PCM -> a raw spectrogram PNG at output_path (absolute).
    device_png: the file is the device encoder's stream (bnhip_spectrogram_png_pcm16) instead of the host's zlib one."""
    if not output_path:
        raise ValueError("output path is empty")
    if not os.path.isabs(output_path):
        raise ValueError("output path must be absolute")
    if len(pcm_bytes) < 2 or len(pcm_bytes) % 2:
        raise ValueError("PCM data must be a non-empty whole number of 16-bit samples")
    clip = np.frombuffer(pcm_bytes, "<i2")
    if device_png:
        _render_png(clip, [output_path], sample_rate, width, profile, style, dynamic_range, device)
        return
    img, pal = _render(clip, sample_rate, width, profile, style, dynamic_range, device)
    write_png(output_path, img[0], pal)


def generate_batch(clips_pcm16, output_paths, width, sample_rate, profile=None, style="default", dynamic_range="100", device=0,
                   device_png=False):
    """Many clips of one length in one device call: int16 [B, n] -> one PNG per clip at output_paths[i].  -> the uint8 [B, H, W] indices.
    device_png: the files are the device encoder's streams, and the returned indices are decoded from them."""
    clips = np.ascontiguousarray(clips_pcm16, np.int16)
    if clips.ndim != 2 or clips.shape[0] != len(output_paths):
        raise ValueError("clips must be int16 [B, n] with one output path per clip")
    for p in output_paths:
        if not p or not os.path.isabs(p):
            raise ValueError("output path must be absolute")
    if device_png:
        return _render_png(clips, output_paths, sample_rate, width, profile, style, dynamic_range, device)
    img, pal = _render(clips, sample_rate, width, profile, style, dynamic_range, device)
    for i, p in enumerate(output_paths):
        write_png(p, img[i], pal)
    return img


def _burst(clips):
    """The clips as contiguous mono int16 arrays and their indices grouped by length, in the order the lengths first appear."""
    clips = [np.ascontiguousarray(c) for c in clips]
    for c in clips:
        if c.dtype != np.int16 or c.ndim != 1 or c.size == 0:
            raise ValueError("clips must be non-empty 1-D int16 arrays")
    groups = {}
    for i, c in enumerate(clips):
        groups.setdefault(c.size, []).append(i)
    return clips, groups


def generate_burst(clips, output_paths, width, sample_rate, profile=None, style="default", dynamic_range="100", device=0,
                   device_png=False, ragged=False):
    """A burst of detections: a sequence of 1-D int16 clips of any lengths -> one PNG per clip at output_paths[i].  -> the uint8
    [B, H, W] indices, in the input's order.  Clips are grouped by length, one generate_batch call per length; ragged: the whole burst
    in one device call (bnhip_spectrogram_ragged_pcm16, or with device_png bnhip_spectrogram_png_ragged_pcm16) instead."""
    clips, groups = _burst(clips)
    if not clips or len(clips) != len(output_paths):
        raise ValueError("a burst is a non-empty sequence of clips with one output path per clip")
    for p in output_paths:
        if not p or not os.path.isabs(p):
            raise ValueError("output path must be absolute")
    if not ragged:
        img = None
        for idx in groups.values():
            part = generate_batch(np.stack([clips[i] for i in idx]), [output_paths[i] for i in idx], width, sample_rate, profile, style,
                                  dynamic_range, device, device_png)
            if img is None:
                img = np.empty((len(clips),) + part.shape[1:], np.uint8)
            img[idx] = part
        return img
    kw = _render_args(sample_rate, width, profile, style, dynamic_range)
    if device_png:
        streams = _host.spectrogram_png_ragged(clips, sample_rate, width, palette(style), device=device, **kw)
        for p, s in zip(output_paths, streams):
            with open(p, "wb") as fh:
                fh.write(s)
        return np.stack([read_png_indices(s) for s in streams])
    img, pal = _host.spectrogram_ragged(clips, sample_rate, width, device=device, **kw), palette(style)
    for i, p in enumerate(output_paths):
        write_png(p, img[i], pal)
    return img


def generate_from_flac(streams, output_paths, width, profile=None, style="default", dynamic_range="100", device=0):
    """GenerateFromFile (generator.go:276-424) for clips saved as FLAC: a sequence of FLAC streams -> one PNG per stream at
    output_paths[i], the counterpart of generate_burst(.., device_png=True, ragged=True) that starts from the saved file.  The streams
    are grouped by sample rate, one device call per rate (bnhip_flac_spectrogram_png: decode, render and PNG-encode, the PCM never
    reaches the host); the files are the device's PNG streams.  -> the streams' statuses (host.FLAC_*), in the input's order; nothing is
    written for a stream whose status is not host.FLAC_OK."""
    streams = [bytes(s) for s in streams]
    if not streams or len(streams) != len(output_paths):
        raise ValueError("a burst is a non-empty sequence of streams with one output path per stream")
    for p in output_paths:
        if not p or not os.path.isabs(p):
            raise ValueError("output path must be absolute")
    infos = [_host.flac_stream_info(s) for s in streams]
    status = [int(i.status) for i in infos]
    groups = {}
    for i, info in enumerate(infos):
        if info.status == _host.FLAC_OK:
            groups.setdefault(int(info.rate), []).append(i)
    for rate, idx in groups.items():
        kw = _render_args(rate, width, profile, style, dynamic_range)
        pngs, results = _host.flac_spectrogram_png([streams[i] for i in idx], width, palette(style), device=device, **kw)
        for i, png, res in zip(idx, pngs, results):
            status[i] = int(res.status)
            if res.status == _host.FLAC_OK:
                with open(output_paths[i], "wb") as fh:
                    fh.write(png)
    return status
