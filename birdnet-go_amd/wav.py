"""WAV/PCM ingest + clip framing feeding the batch API (SURVEY.md section 8f "next" row 1).

Formats follow the reference's converters (`internal/audiocore/convert/pcm.go:206-268`: 16/24/32-bit
little-endian integer PCM -> float32 by /32768, /8388608, /2147483648; WAVE_FORMAT_EXTENSIBLE with the
PCM sub-format is what `tawnyowl.wav` uses).  Framing follows the documented file-analysis behaviour
(`doc/wiki/file-analysis.md:1-44`, flags `cmd/root.go:93-95`): consecutive `clip_len` windows advanced by
`clip_len - overlap`; the final partial window is zero-padded to full length (kept if it holds at
least `min_tail` seconds of audio).  Host-side numpy; the conversion arithmetic is restated here
independently of the oracle (product code must not import oracle/).
"""
import math
import struct

import numpy as np


class WavError(ValueError):
    pass


def _first_channel(path_or_bytes):
    """-> (first channel's sample bytes uint8 [n, bits / 8], sample_rate, bit_depth)."""
    data, rate, bits, channels = _data_chunk(path_or_bytes)
    bps = bits // 8
    n = len(data) // (bps * channels)
    return np.frombuffer(data, np.uint8, n * bps * channels).reshape(n, channels, bps)[:, 0, :], rate, bits


def read_wav_frames(path_or_bytes):
    """-> (the whole frames of the data chunk as they are in the file - the channels interleaved, little-endian, bit_depth / 8 bytes a
    sample -, sample_rate, bit_depth, channels): what the multichannel analysis sends (`HipClassifier.analyze_channels_pcm`), which
    picks or mixes the channels on the device.  No pass over the samples is made here."""
    data, rate, bits, channels = _data_chunk(path_or_bytes)
    frame = (bits // 8) * channels
    return data[:len(data) // frame * frame], rate, bits, channels


def _data_chunk(path_or_bytes):
    """-> (the data chunk's bytes, sample_rate, bit_depth, channels) of an integer-PCM WAV file."""
    raw = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    if len(raw) < 12 or raw[:4] != b"RIFF" or raw[8:12] != b"WAVE":
        raise WavError("not a RIFF/WAVE file")
    pos, fmt, data = 12, None, None
    while pos + 8 <= len(raw):
        cid, size = raw[pos:pos + 4], struct.unpack_from("<I", raw, pos + 4)[0]
        body = raw[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            fmt = body
        elif cid == b"data":
            data = body
            break
        pos += 8 + size + (size & 1)
    if fmt is None or data is None or len(fmt) < 16:
        raise WavError("missing fmt/data chunk")
    tag, channels, rate, _, block_align, bits = struct.unpack_from("<HHIIHH", fmt, 0)
    if tag == 0xFFFE:                               # WAVE_FORMAT_EXTENSIBLE: sub-format GUID's first word is the real tag
        if len(fmt) < 40:
            raise WavError("truncated extensible fmt chunk")
        tag = struct.unpack_from("<H", fmt, 24)[0]
    if tag != 1:
        raise WavError(f"unsupported WAV format tag {tag} (integer PCM only)")
    if bits not in (16, 24, 32) or channels < 1:
        raise WavError(f"unsupported audio bit depth: {bits}")
    return data, int(rate), int(bits), int(channels)


def read_wav_pcm(path_or_bytes):
    """-> (the first channel's PCM bytes as they are in the file (little-endian, bit_depth / 8 each), sample_rate, bit_depth): what
    the device-framed analysis sends (`HipClassifier.analyze_pcm`), converted on the device exactly as read_wav converts."""
    b, rate, bits = _first_channel(path_or_bytes)
    return np.ascontiguousarray(b).tobytes(), rate, bits


def read_wav(path_or_bytes):
    """-> (samples float32 [n] (first channel), sample_rate, bit_depth)."""
    b, rate, bits = _first_channel(path_or_bytes)
    n = b.shape[0]
    if bits == 16:
        s = b.copy().view("<i2").reshape(n).astype(np.float32) / np.float32(32768.0)
    elif bits == 24:
        v = (b[:, 0].astype(np.int32) | (b[:, 1].astype(np.int32) << 8) | (b[:, 2].astype(np.int32) << 16))
        v = np.where(v & 0x800000, v | ~0xFFFFFF, v).astype(np.int32)
        s = v.astype(np.float32) / np.float32(8388608.0)
    else:
        s = b.copy().view("<i4").reshape(n).astype(np.float32) / np.float32(2147483648.0)
    return s, rate, bits


def _framing(sample_rate, clip_seconds, overlap_seconds, min_tail_seconds):
    clip_len = int(round(clip_seconds * sample_rate))
    hop = clip_len - int(round(overlap_seconds * sample_rate))
    if clip_len <= 0 or hop <= 0:
        raise ValueError("overlap must be smaller than the clip length")
    return clip_len, hop, int(min_tail_seconds * sample_rate)


def window_table(lengths, sample_rate, clip_seconds=3.0, overlap_seconds=0.0, min_tail_seconds=1.0):
    """frame_clips' rule for recordings of `lengths` samples, without the samples (bnhip_analyze_windows; needs no device):
    -> (first_window int64 [n + 1], clip_len, hop, min_tail).  Recording r owns windows first_window[r] .. first_window[r + 1] - 1
    of the burst; its window j starts at sample j * hop."""
    from . import host
    clip_len, hop, min_tail = _framing(sample_rate, clip_seconds, overlap_seconds, min_tail_seconds)
    return host.analyze_windows(lengths, clip_len, hop, min_tail), clip_len, hop, min_tail


def frame_clips(samples, sample_rate, clip_seconds=3.0, overlap_seconds=0.0, min_tail_seconds=1.0):
    """-> (clips float32 [n_clips, clip_len], start_times_seconds [n_clips])."""
    clip_len, hop, min_tail = _framing(sample_rate, clip_seconds, overlap_seconds, min_tail_seconds)
    x = np.asarray(samples, np.float32).reshape(-1)
    starts = []
    p = 0
    while p < x.size:
        remain = x.size - p
        if remain >= clip_len or remain >= min_tail or not starts:
            starts.append(p)
        if remain <= clip_len:
            break
        p += hop
    clips = np.zeros((len(starts), clip_len), np.float32)
    for i, s0 in enumerate(starts):
        seg = x[s0:s0 + clip_len]
        clips[i, :seg.size] = seg
    return clips, np.asarray(starts, np.float64) / sample_rate


def analyze_file(path, classifier, labels=None, sensitivity=1.0, overlap_seconds=0.0, top_k=10, threshold=0.0,
                 model_rate=48000, device=0, device_framing=False, device_resample=False, channels=None, return_chosen=False):
    """File analysis = read -> (resample to the model's rate) -> frame -> batched predict_topk.
    Returns rows (start_s, end_s, label|index, confidence).

    `model_rate` is the sample rate the classifier's clip length is expressed in (48 kHz for BirdNET v2.4,
    `internal/classifier/model_registry.go:138-153`).  A file at another rate is resampled on the GPU first, as the
    reference resamples file input to the model rate (`internal/audiocore/resample/resample.go`, call sites
    `analysis/buffer_consumer.go:118,192`); window times are in seconds of audio, whatever the file's rate.

    device_framing=True: the same rows from one `bnhip_analyze_pcm` call - the file's PCM bytes go to the device as they are
    and the windows are framed there (a resampled file goes as float32; with device_resample=True it too goes as it is and is
    resampled on the device, see analyze_files).

    channels (a channel index, "mix" or "auto"; analyze_files): the file's frames go interleaved and the channel is picked or mixed
    on the device, in the device-framed call; return_chosen=True then answers (rows, the channel read or "mix")."""
    if channels is not None:
        rows, chosen = analyze_files([path], classifier, labels, sensitivity, overlap_seconds, top_k, threshold, model_rate, device,
                                     channels=channels, return_chosen=True)
        return (rows[0], chosen[0]) if return_chosen else rows[0]
    if device_framing:
        return analyze_files([path], classifier, labels, sensitivity, overlap_seconds, top_k, threshold, model_rate, device,
                             device_resample=device_resample)[0]
    s, rate, _ = read_wav(path)
    if model_rate <= 0:
        raise WavError(f"invalid model sample rate {model_rate}")
    if rate != model_rate:
        from . import host                               # GPU resampler (bnhip_resample_f32); fails loudly without a device
        s = host.Resampler(rate, model_rate, device=device).resample_f32(s)
    clip_seconds = classifier.n_samples / float(model_rate)
    clips, starts = frame_clips(s, model_rate, clip_seconds, overlap_seconds)
    if clips.shape[1] != classifier.n_samples:
        raise WavError(f"framed clip length {clips.shape[1]} != model input {classifier.n_samples}")
    conf, idx = classifier.predict_topk(clips.reshape(-1), clips.shape[0], k=top_k, sensitivity=sensitivity)
    rows = []
    for i in range(clips.shape[0]):
        for c, j in zip(conf[i], idx[i]):
            if c >= threshold:
                rows.append((float(starts[i]), float(starts[i] + clip_seconds), labels[j] if labels else int(j), float(c)))
    return rows


def _round_down_f32(v):
    """The float32 t with `x > t` true for exactly the float32 x with `x > v` in float64: v rounded DOWN (toward -inf).  No float32
    lies between t and v, so the strict test keeps the same rows; rounding to nearest could land above v and drop a confidence
    that lies between.  (The mirror of the >= threshold of the rows, which is rounded up.)"""
    v = float(v)
    t = np.float32(v)
    if not np.isfinite(t):
        return t if not np.isfinite(v) or v < 0 else np.float32(np.finfo(np.float32).max)      # (a finite v beyond float32's range)
    return np.nextafter(t, np.float32(-np.inf)) if float(t) > v else t


class EventFilter:
    """The reference's result post-filters for analyze_files(events=...): which hits count and how they merge into detection events
    (include/bnhip.h, "Detection events").

    default_threshold, thresholds {class index: value}: a hit is confidence > its class's threshold.  include (indices; every other
    class is excluded) and exclude (indices).  veto (indices): classes whose hits above veto_threshold drop the events that began
    in the hold before them (the privacy filter's human voice) and that form no events themselves.  hold_seconds: how long an
    event stays open after its first hit.  min_count: the hits an event needs; or level (0-5): the reference's false-positive filter
    level, from which the count follows at the call's overlap.  keep_dropped: answer the dropped events too, with their status."""

    def __init__(self, default_threshold=0.8, thresholds=None, include=None, exclude=(), veto=(), veto_threshold=0.0, hold_seconds=15.0,
                 min_count=None, level=None, keep_dropped=False):
        if min_count is not None and level is not None:
            raise ValueError("min_count or level, not both")
        self.default_threshold, self.thresholds = float(default_threshold), dict(thresholds or {})
        self.include, self.exclude, self.veto = (None if include is None else list(include)), list(exclude), list(veto)
        self.veto_threshold, self.hold_seconds = float(veto_threshold), float(hold_seconds)
        self.min_count, self.level, self.keep_dropped = min_count, level, bool(keep_dropped)

    def hold_windows(self, model_rate, hop):
        return max(1, int(math.ceil(self.hold_seconds * model_rate / hop)))

    def tables(self, n_classes, model_rate, hop, overlap_seconds=0.0):
        """-> the host.EventTables of this filter for a model of n_classes classes analysed at `hop` samples of model_rate."""
        from . import host
        thr = np.full(n_classes, _round_down_f32(self.default_threshold), np.float32)
        for j, v in self.thresholds.items():
            thr[j] = _round_down_f32(v)
        if self.include is not None:
            out = np.ones(n_classes, bool)
            out[self.include] = False
            thr[out] = np.inf
        thr[self.exclude] = np.inf
        veto = None
        if self.veto:
            veto = np.zeros(n_classes, np.uint8)
            veto[self.veto] = 1
        if self.level is not None:
            min_count = host.event_min_count(self.level, overlap_seconds)
        else:
            min_count = 1 if self.min_count is None else int(self.min_count)
        return host.EventTables(thr, veto, _round_down_f32(self.veto_threshold), self.hold_windows(model_rate, hop), min_count,
                                host.EVENTS_KEEP_DROPPED if self.keep_dropped else 0)


class ExtendedCapture:
    """The reference's extended capture for analyze_files(events=..., extend=...) and stream.WindowBatcher(events=..., extend=...)
    (include/bnhip.h, "Detection events: extended capture"): every new hit of an event of the chosen species moves the event's
    deadline - short_wait_seconds (or the filter's hold, if longer) behind the hit while the event is younger than
    medium_after_seconds, medium_wait_seconds while it is younger than long_after_seconds, long_wait_seconds after that - and
    max_seconds behind the event's first hit is the latest.  species: None for every class, or class indices."""

    def __init__(self, species=None, max_seconds=None, short_wait_seconds=15.0, medium_after_seconds=30.0, medium_wait_seconds=30.0,
                 long_after_seconds=120.0, long_wait_seconds=60.0):
        if max_seconds is None:
            raise ValueError("extended capture needs max_seconds")
        self.species = None if species is None else list(species)
        self.max_seconds, self.short_wait_seconds = float(max_seconds), float(short_wait_seconds)
        self.medium_after_seconds, self.medium_wait_seconds = float(medium_after_seconds), float(medium_wait_seconds)
        self.long_after_seconds, self.long_wait_seconds = float(long_after_seconds), float(long_wait_seconds)

    def tables(self, n_classes, model_rate, hop):
        """-> the host.EventExtend for a model of n_classes classes analysed at `hop` samples of model_rate: seconds become windows
        as EventFilter.hold_windows makes them, with a ceiling."""
        from . import host
        table = None
        if self.species is not None:
            table = np.zeros(n_classes, np.uint8)
            table[self.species] = 1
        w = lambda seconds: max(1, int(math.ceil(seconds * model_rate / hop)))
        return host.EventExtend(table, w(self.max_seconds), w(self.short_wait_seconds), w(self.medium_after_seconds), w(self.medium_wait_seconds),
                                w(self.long_after_seconds), w(self.long_wait_seconds))


# the reference's dog classes (vocalization_labels.go): BirdNET's "Dog_<localised name>" by its prefix, Perch v2's by their names
DOG_LABEL_PREFIX = "dog_"
DOG_LABELS = ("dog", "bark", "growling", "canis familiaris")


def is_dog_label(label):
    """isDogDetection: whether a raw classifier label is a dog class for the dog-bark filter (case-insensitive)."""
    low = str(label).lower()
    return low in DOG_LABELS or low.startswith(DOG_LABEL_PREFIX)


class EventGuards:
    """The reference's dog-bark and daylight filters for analyze_files(events=..., guards=...) (include/bnhip.h, "Detection events:
    dog-bark and daylight filters").

    Dog bark: a result of a dog class above `confidence` marks its window; an event of one of `species` whose deadline lies at most
    remember_minutes behind the last such window before it is dropped (status host.EVENT_DOG).  dog_labels: the dog classes as
    indices, or None to find them among the labels passed to tables() by the reference's rule (is_dog_label).  Daylight: an event of
    one of daylight_species whose first window begins inside a daylight interval of its file is dropped (host.EVENT_DAYLIGHT).
    daylight: {path: [(from_seconds, to_seconds), ...]} in seconds from the recording's start, ascending and disjoint (the host's
    civil dawn + offset and civil dusk - offset; a path without an entry has no daylight: the filter fails open).  species and
    daylight_species hold class indices, or labels when tables() is given labels.

    Windows: remember_minutes becomes ceil(minutes * 60 * rate / hop) windows, as the hold does.  Window w begins at w * hop / rate
    seconds and is in daylight when that instant lies in [from, to): both edges are rounded up to the next window start,
    ceil(seconds * rate / hop)."""

    def __init__(self, confidence, species=(), remember_minutes=5.0, dog_labels=None, daylight_species=(), daylight=None):
        self.confidence, self.species, self.remember_minutes = float(confidence), list(species), float(remember_minutes)
        self.dog_labels = None if dog_labels is None else list(dog_labels)
        self.daylight_species, self.daylight = list(daylight_species), dict(daylight or {})
        if self.remember_minutes < 0:
            raise ValueError("remember_minutes must not be negative")

    def tables(self, n_classes, model_rate, hop, labels=None, paths=()):
        """-> the host.EventGuards for a model of n_classes classes analysed at `hop` samples of model_rate; paths: the call's
        files in order, whose daylight intervals become the spans of recordings 0, 1, ..."""
        from . import host

        def table(items):
            t = np.zeros(n_classes, np.uint8)
            for it in items:
                if isinstance(it, str):
                    if labels is None or it not in labels:
                        raise ValueError(f"unknown species label: {it!r}")
                    it = list(labels).index(it)
                t[int(it)] = 1
            return t if t.any() else None

        if self.dog_labels is not None:
            dog = table(self.dog_labels)
        else:
            dog = table([j for j, name in enumerate(labels or ()) if j < n_classes and is_dog_label(name)])
        edge = lambda seconds: max(0, int(math.ceil(seconds * model_rate / hop)))
        spans = []
        for r, path in enumerate(paths):
            last = 0
            for lo, hi in self.daylight.get(path, ()):
                lo, hi = edge(lo), edge(hi)
                if lo < last:
                    raise ValueError(f"{path}: daylight intervals must ascend and not overlap")
                if hi > lo:                                               # (an interval that holds no window start drops nothing)
                    spans.append((r, lo, hi))
                    last = hi
        remember = int(math.ceil(self.remember_minutes * 60.0 * model_rate / hop))
        return host.EventGuards(dog, _round_down_f32(self.confidence), table(self.species), remember, table(self.daylight_species),
                                np.array(spans, np.int32).reshape(-1, 3) if spans else None)


class ClipExport:
    """What analyze_files(events=..., export=...) saves of every detection event, as the reference does for an approved detection
    (include/bnhip.h, "Detection clips"): the clip from pre_capture_seconds before the event's first window to length_seconds -
    pre_capture_seconds behind it - with extended=True behind the event's LAST window, the clip then cut at max_seconds (required) -
    loudness-normalised (normalize, target_lufs, true_peak_dbtp, max_gain_db, gate_fallback), FLAC-encoded (lpc_order,
    seek_seconds: a seek point every so many seconds, 0 = none) and, with image=(width, height) and a palette, rendered to a
    spectrogram PNG at rate_out (window, top_db, range_db as host.spectrogram_png_ragged takes them).  max_clips: the clips one
    call has room for; the events behind them come back without a clip."""

    def __init__(self, length_seconds=15.0, pre_capture_seconds=3.0, extended=False, max_seconds=None, normalize=True, target_lufs=-23.0,
                 true_peak_dbtp=-1.0, max_gain_db=30.0, gate_fallback=False, lpc_order=8, seek_seconds=0.0, image=None, palette=None,
                 rate_out=0, window=None, top_db=0.0, range_db=100.0, max_clips=256):
        if extended and max_seconds is None:
            raise ValueError("extended capture needs max_seconds")
        if image is not None and palette is None:
            raise ValueError("an image needs a palette")
        self.length_seconds, self.pre_capture_seconds, self.extended = float(length_seconds), float(pre_capture_seconds), bool(extended)
        self.max_seconds = None if max_seconds is None else float(max_seconds)
        self.normalize, self.target_lufs, self.true_peak_dbtp = bool(normalize), float(target_lufs), float(true_peak_dbtp)
        self.max_gain_db, self.gate_fallback, self.lpc_order, self.seek_seconds = float(max_gain_db), bool(gate_fallback), int(lpc_order), float(seek_seconds)
        self.image, self.palette, self.rate_out, self.window = image, palette, int(rate_out), window
        self.top_db, self.range_db, self.max_clips = float(top_db), float(range_db), int(max_clips)

    def settings(self, model_rate):
        """-> the host.ClipSettings of this export at model_rate: seconds become samples, rounded to nearest."""
        from . import host
        pre = int(round(self.pre_capture_seconds * model_rate))
        post = int(round(self.length_seconds * model_rate)) - pre
        most = 2 ** 31 - 1 if self.max_seconds is None else int(round(self.max_seconds * model_rate))
        width, height = self.image if self.image is not None else (0, None)
        return host.ClipSettings(pre, post, most, self.extended, self.normalize, self.target_lufs, self.true_peak_dbtp, self.max_gain_db,
                                 self.gate_fallback, int(round(self.seek_seconds * model_rate)), self.lpc_order, width, self.rate_out, self.window,
                                 self.top_db, self.range_db, self.palette, height)


def clip_spans(events, resampled_length, hop, export, model_rate=48000):
    """The span rule of ClipExport alone (bnhip_event_clip_spans, host only): events (host.EVENT) of recordings of `resampled_length`
    samples at model_rate, analysed at `hop` -> host.CLIP_SPAN [n_events] (start, length in samples; length 0 for a dropped event)."""
    from . import host
    return host.event_clip_spans(events, resampled_length, hop, export.settings(model_rate))


def _is_flac(p):
    return p[:4] == b"fLaC" if isinstance(p, (bytes, bytearray)) else str(p).lower().endswith(".flac")


def _name(p):
    return f"<{len(p)} bytes>" if isinstance(p, (bytes, bytearray)) else str(p)


def _flac_results(paths, results):
    """A recording the device decoder did not find whole is an error of the call, by name."""
    for p, r in zip(paths, results):
        if int(r["status"]) != 0:
            raise WavError(f"{_name(p)}: damaged FLAC stream: frame {int(r['frames'])} at byte {int(r['fail_offset'])} does not decode")


def analyze_files(paths, classifier, labels=None, sensitivity=1.0, overlap_seconds=0.0, top_k=10, threshold=0.0, model_rate=48000,
                  device=0, device_resample=False, channels=None, return_chosen=False, events=None, export=None, extend=None, guards=None):
    """analyze_file(device_framing=True) for a burst of recordings in ONE device call (`bnhip_analyze_pcm`): -> one list of rows per
    path, each what analyze_file returns for that file.  The files' PCM bytes are sent as they are when all of them are at the
    model's rate and share one bit depth; otherwise every file goes as float32 (converted, and resampled where its rate differs,
    exactly as analyze_file does).

    device_resample=True: every file's bytes go as they are, whatever its rate and depth, in one `bnhip_analyze_mixed_pcm` call
    that resamples and converts them on the device - the same rows.

    channels: None analyses every file's first channel, de-interleaved here on the host (the paths above).  A channel index, "mix"
    or "auto" sends every file's frames interleaved as they are, whatever its rate, depth and channel count, in one
    `bnhip_analyze_channels_pcm` call: that channel, the mean of the channels, or - decided per file on the device from the
    channels' energies, by the reference's rule - one of the two.  return_chosen=True (with channels set): -> (rows, chosen), chosen
    the channel read of every file, or "mix".

    events (an EventFilter): every route above answers detection events instead of rows, merged on the device in the same call
    (`bnhip_analyze_*_pcm_events`; `threshold` gives way to the filter's own): per path a list of (start_s, end_s, label | index,
    confidence, count), and with keep_dropped also the status; start = first_window * hop / rate, end = last_window * hop / rate +
    the clip.

    export (a ClipExport, with events; keep_dropped is refused): the same call also makes every event's clip on the device
    (`bnhip_analyze_channels_pcm_clips`: every file's frames go up interleaved as they are - channels=None reads channel 0 there).
    Each tuple is followed by the clip's start and length in samples at model_rate, its FLAC bytes, its loudness record
    (host.Loudness, None without normalize) and its PNG bytes or None; an event behind the export's max_clips has None for all three.

    extend (an ExtendedCapture, with events): the events of its species last as long as the bird kept calling
    (`bnhip_analyze_channels_pcm_events_extended`, `bnhip_analyze_channels_pcm_clips_extended`); the call takes the channels route, as
    with export, and an export with extended=True then cuts every clip to its event's last hit.

    guards (an EventGuards, with events): the reference's dog-bark and daylight filters run on the device behind the other two
    (`bnhip_analyze_channels_pcm_events_guarded`, `bnhip_analyze_channels_pcm_clips_guarded`), with or without an extend; the call
    takes the channels route.  A dropped event is left out - with keep_dropped it comes with status host.EVENT_DOG or
    host.EVENT_DAYLIGHT - and gets no clip.  `labels` is where the dog classes are looked for.

    FLAC recordings (paths ending in .flac, or bytes that start with fLaC; 1 or 2 channels, 16 or 24 bits), with channels set: the
    compressed files go to the device as they are and are decoded there, in one `bnhip_analyze_flac` / `bnhip_analyze_flac_events`
    call - the same rows as the same audio in WAV files.  A burst that holds a FLAC file takes FLAC files only; a file the decoder
    finds damaged raises WavError naming it and the offset; export, extend and guards are not offered for FLAC files."""
    if model_rate <= 0:
        raise WavError(f"invalid model sample rate {model_rate}")
    if return_chosen and channels is None:
        raise ValueError("return_chosen needs channels")
    if export is not None and (events is None or events.keep_dropped):
        raise ValueError("export needs events, without keep_dropped")
    if extend is not None and events is None:
        raise ValueError("extend needs events")
    if guards is not None and events is None:
        raise ValueError("guards need events")
    recs = crecs = flac = None
    if any(_is_flac(p) for p in paths):
        if export is not None or extend is not None or guards is not None:
            raise ValueError("export=, extend= and guards= are not offered for FLAC recordings: decode them (flac.decode_recordings) or use WAV files")
        if channels is None:
            raise ValueError("FLAC recordings are analysed with channels set (a channel index, \"mix\" or \"auto\")")
        for p in paths:
            if not _is_flac(p):
                raise WavError(f"a burst that holds FLAC recordings takes FLAC recordings only: {_name(p)} is not one")
        flac = [bytes(p) if isinstance(p, (bytes, bytearray)) else open(p, "rb").read() for p in paths]
    # (the export and the extend take the files' frames: channel 0 is read there)
    select = 0 if channels is None and (export is not None or extend is not None or guards is not None) else channels
    if select is None:
        pcm = [read_wav_pcm(p) for p in paths]
        depths = {bits for _, _, bits in pcm}
    if flac is not None:
        bufs, lengths = flac, None                        # (the lengths in samples are STREAMINFO's, read by the call)
    elif select is not None:
        from . import host
        frames = [read_wav_frames(p) for p in paths]
        bufs = [raw for raw, _, _, _ in frames]
        lengths = [len(raw) // ((bits // 8) * ch) for raw, _, bits, ch in frames]
        crecs = host.channel_recordings(lengths, [f[1] for f in frames], [f[2] for f in frames], [f[3] for f in frames], select)
    elif device_resample:
        from . import host
        bufs = [raw for raw, _, _ in pcm]
        lengths = [len(raw) // (bits // 8) for raw, _, bits in pcm]
        recs = host.recordings(lengths, [rate for _, rate, _ in pcm], [bits for _, _, bits in pcm])
    elif len(depths) == 1 and all(rate == model_rate for _, rate, _ in pcm):
        bits, bufs = depths.pop(), [raw for raw, _, _ in pcm]
        lengths = [len(raw) // (bits // 8) for raw in bufs]
    else:
        bits, bufs = 0, []
        for p in paths:
            s, rate, _ = read_wav(p)
            if rate != model_rate:
                from . import host
                s = host.Resampler(rate, model_rate, device=device).resample_f32(s)
            bufs.append(np.ascontiguousarray(s, np.float32).tobytes())
        lengths = [len(raw) // 4 for raw in bufs]
    if not bufs or (lengths is not None and min(lengths) < 1):
        raise WavError("a recording without samples")
    clip_seconds = classifier.n_samples / float(model_rate)
    clip_len, hop, min_tail = _framing(model_rate, clip_seconds, overlap_seconds, 1.0)
    if clip_len != classifier.n_samples:
        raise WavError(f"framed clip length {clip_len} != model input {classifier.n_samples}")
    # the rows' test is `float32 confidence >= threshold`: on the device the threshold is a float32, so it is rounded UP - no float32
    # lies between the two, and the test keeps exactly the rows the float64 comparison keeps
    t32 = np.float32(threshold)
    if float(t32) < threshold:
        t32 = np.nextafter(t32, np.float32(np.inf))
    if events is not None:
        flt = events.tables(classifier.num_species(),model_rate, hop, overlap_seconds)
        ext = None if extend is None else extend.tables(classifier.num_species(), model_rate, hop)
        gds = None if guards is None else guards.tables(classifier.num_species(), model_rate, hop, labels, list(paths))
        chosen = clips = None
        if export is not None:
            clips = classifier.analyze_channels_pcm_clips(b"".join(bufs), crecs, model_rate, hop, flt, export.settings(model_rate), min_tail,
                                                          k=top_k, sensitivity=sensitivity, max_clips=export.max_clips, extend=ext,
                                                          guards=gds)
            ev, chosen = clips.events, ["mix" if s < 0 else int(s) for s in clips.chosen]
        elif flac is not None:
            ev, sel, res = classifier.analyze_flac_events(flac, select, model_rate, hop, flt, min_tail, k=top_k, sensitivity=sensitivity)
            _flac_results(paths, res)
            chosen = ["mix" if s < 0 else int(s) for s in sel]
        elif crecs is not None:
            ev, sel = classifier.analyze_channels_pcm_events(b"".join(bufs), crecs, model_rate, hop, flt, min_tail, k=top_k, sensitivity=sensitivity,
                                                             extend=ext, guards=gds)
            chosen = ["mix" if s < 0 else int(s) for s in sel]
        elif recs is not None:
            ev = classifier.analyze_mixed_pcm_events(b"".join(bufs), recs, model_rate, hop, flt, min_tail, k=top_k, sensitivity=sensitivity)
        else:
            ev = classifier.analyze_pcm_events(b"".join(bufs), bits, lengths, hop, flt, min_tail, k=top_k, sensitivity=sensitivity)
        out = [[] for _ in paths]
        nc = 0                                        # the clip of the next event with a span (clips are made in event order)
        for i, e in enumerate(ev):
            start = np.float64(int(e["first_window"]) * hop) / model_rate
            end = np.float64(int(e["last_window"]) * hop) / model_rate + clip_seconds
            j = int(e["class_index"])
            row = (float(start), float(end), labels[j] if labels else j, float(e["confidence"]), int(e["count"]))
            if clips is not None:
                sp = clips.spans[i]
                has = int(sp["length"]) > 0 and nc < clips.n_clips
                row += (int(sp["start"]), int(sp["length"]), clips.flac[nc] if has else None,
                        clips.loudness[nc] if has and clips.loudness is not None else None, clips.png[nc] if has and clips.png is not None else None)
                nc += 1 if int(sp["length"]) > 0 else 0
            out[int(e["recording"])].append(row + (int(e["status"]),) if events.keep_dropped else row)
        return (out, chosen) if return_chosen else out
    chosen = None
    if flac is not None:
        det, _, sel, res = classifier.analyze_flac(flac, select, model_rate, hop, min_tail, k=top_k, sensitivity=sensitivity, threshold=float(t32))
        _flac_results(paths, res)
        chosen = ["mix" if s < 0 else int(s) for s in sel]
    elif crecs is not None:
        det, _, sel = classifier.analyze_channels_pcm(b"".join(bufs), crecs, model_rate, hop, min_tail, k=top_k, sensitivity=sensitivity,
                                                      threshold=float(t32))
        chosen = ["mix" if s < 0 else int(s) for s in sel]
    elif recs is not None:
        det, _ = classifier.analyze_mixed_pcm(b"".join(bufs), recs, model_rate, hop, min_tail, k=top_k, sensitivity=sensitivity, threshold=float(t32))
    else:
        det, _ = classifier.analyze_pcm(b"".join(bufs), bits, lengths, hop, min_tail, k=top_k, sensitivity=sensitivity, threshold=float(t32))
    out = [[] for _ in paths]
    for r, w, j, c in zip(det["recording"], det["window"], det["class_index"], det["confidence"]):
        start = np.float64(int(w) * hop) / model_rate
        out[int(r)].append((float(start), float(start + clip_seconds), labels[j] if labels else int(j), float(c)))
    return (out, chosen) if return_chosen else out
