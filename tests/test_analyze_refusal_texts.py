"""Which text every device entry of the file-analysis family answers a bad argument with, and - where two arguments are bad - which
of the two is answered: a table of (entry, broken arguments) -> (code, bnhip_last_error() text).  The tests beside this one
(test_analyze*_ref.py) pin that such calls are refused before the handle or a device is looked at; this one pins the words and their
order, so that the entries' bodies can be rearranged without the answers moving.  The expected texts are literals, recorded from the
library as it was before the family's entries were restated.  No device: plan-only handles, and the device-ordinal entries only ever
with an argument they refuse."""
import ctypes as C

import numpy as np

from birdnet_go_amd import host

from test_analyze_channels_ref import _bad_channel_tables, ch_recs
from test_analyze_mixed_ref import _bad_tables

RATE = 48000
NULL, RANGE, RATE0 = "NULL argument", "n_recordings must be in [1, 65535]", "model_rate must be positive"
HOP, TAIL = "hop must be in [1, n_samples]", "min_tail must not be negative"
DEPTH8 = "unsupported bit depth: 8 (supported: 0 = float32, 16, 24, 32)"
NO_SAMPLES, BURST = "every recording needs at least one sample", "burst of 2^36 samples or more"
FILTER, HOLD, MIN_COUNT, FLAGS = "NULL event filter / class_threshold", "hold_windows must be at least 1", "min_count must be at least 1", "unknown event filter flags"
PLAN_ONLY, SINGLE, ROWS = "plan-only model cannot run", "file analysis runs on one device; use a single-device handle", "2^31 detection rows or more"
AUTO_FLOAT = "the channel energies are measured on integer depths; a float32 recording takes a channel or the mix"
SELECT = "select must be a channel index, BNHIP_CHANNEL_MIX or BNHIP_CHANNEL_AUTO"

# what _bad_tables() of test_analyze_mixed_ref.py is answered with: by the mixed entries, and by the channels entries for the same
# table as stereo
BAD_TABLE = {"rate 0": "recording 2: the sample rate must be positive", "rate < 0": "recording 0: the sample rate must be positive",
             "model_rate 0": RATE0, "model_rate < 0": RATE0,
             "depth 8": "recording 2: " + DEPTH8, "depth -16": "recording 0: unsupported bit depth: -16 (supported: 0 = float32, 16, 24, 32)",
             "depth 64": "recording 2: unsupported bit depth: 64 (supported: 0 = float32, 16, 24, 32)",
             "no samples": NO_SAMPLES, "negative length": NO_SAMPLES, "length 2^31": "recording 2: 2^31 samples or more",
             "n_out 2^31": "recording 2: 2^31 samples or more at the model's rate", "input total 2^36": BURST, "output total 2^36": BURST}
# (as stereo, 17 recordings of 2^31 - 1 frames already hold 2^36 samples: same text, answered by the channels' own count)
# what _bad_channel_tables() of test_analyze_channels_ref.py is answered with
BAD_CHANNELS = {"no channel": "recording 2: channels must be in [1, 16]", "17 channels": "recording 0: channels must be in [1, 16]",
                "negative channels": "recording 2: channels must be in [1, 16]", "select = channels": "recording 2: " + SELECT,
                "select -3": "recording 2: " + SELECT, "select 1 of a mono recording": "recording 2: " + SELECT,
                "auto on float32": "recording 2: " + AUTO_FLOAT, "auto on mono float32": "recording 0: " + AUTO_FLOAT,
                "2^36 samples in 3 * 2^31 frames": BURST}
# the argument errors every analysis entry shares, whatever its form and answer
SHARED = {"h=None": NULL, "x=None": NULL, "table=None": NULL, "nr=0": RANGE, "nr=65536": RANGE, "hop=0": HOP, "hop=n+1": HOP, "mt=-1": TAIL,
          "k=0": "k must be positive", "act=3": "unknown activation"}
ANSWER = {"topk": {"oc=None": NULL, "oi=None": NULL},
          "rows": {"no=None": NULL, "o=None": NULL},
          "events": {"no=None": NULL, "o=None": NULL, "filter=None": FILTER, "thr=None": FILTER, "hold=0": HOLD, "min_count=0": MIN_COUNT,
                     "flags=2": FLAGS,
                     "bad filter + k=0": HOLD,                            # the filter is answered first
                     "plan-only + 2^31 rows": ROWS}}                      # the row bound is an argument error: before the handle
FORM = {"plain": {"bits=8": DEPTH8, "bits=-16": "unsupported bit depth: -16 (supported: 0 = float32, 16, 24, 32)", "length 0": NO_SAMPLES,
                  "bad depth + bad hop": DEPTH8},                         # the depth first
        "mixed": {"bad depth + bad hop": "recording 0: " + DEPTH8, "bad depth + model_rate=0": RATE0},
        "channels": {"bad depth + bad hop": "recording 0: " + DEPTH8, "bad channels + model_rate=0": "recording 0: channels must be in [1, 16]"}}
# bnhip_analyze_channels_pcm_clips: the export settings first, then the filter, then what the channels events entry answers
CLIPS = {"x=None": NULL, "out=None": NULL, "spans=None": NULL, "flac_offsets=None": NULL, "events=None": NULL, "loudness=None": NULL,
         "pre=-1": "pre_samples must not be negative", "post=0": "post_samples must be at least 1", "max=0": "max_samples must be at least 1",
         "lpc=9": "lpc_order must be in [0, 8]", "seek=-1": "seek_interval must not be negative", "rate=0": "sample rate must be in [1, 1048575]",
         "filter=None": FILTER, "thr=None": FILTER, "hold=0": HOLD, "min_count=0": MIN_COUNT, "flags=2": FLAGS,
         "flags=KEEP_DROPPED": "the clip export takes kept events only: BNHIP_EVENTS_KEEP_DROPPED is refused",
         "bad filter + k=0": HOLD, "bad settings + bad filter": "lpc_order must be in [0, 8]",
         "bad channels + model_rate=0": "sample rate must be in [1, 1048575]",      # (here the rate is the export's to answer first)
         "bad depth + bad hop": "recording 0: " + DEPTH8, "plan-only + 2^31 rows": ROWS}
SPANS = {"x=None": NULL, "spans=None": NULL, "out=None": NULL, "rate=0": RATE0, "n_spans=0": "n_spans must be in [1, 65535]",
         "n_spans=65536": "n_spans must be in [1, 65535]", "span recording=2": "span 1: recording outside the table",
         "span recording=-1": "span 1: recording outside the table", "span length=-1": "span 1: negative length",
         "span start=-1": "span 1: outside its recording", "span past the end": "span 1: outside its recording",
         "bad channels + model_rate=0": "recording 0: channels must be in [1, 16]", "bad depth + bad span": "recording 0: " + DEPTH8,
         "x=None + bad table": NULL}
ENERGY_DEPTH = "unsupported bit depth: %d (supported: 16, 24, 32)"
ENERGY = {"x=None": NULL, "table=None": NULL, "o=None": NULL, "nr=0": RANGE, "nr=65536": RANGE,
          "float32": "recording 0: " + AUTO_FLOAT, "depth 8": "recording 0: " + ENERGY_DEPTH % 8, "depth 64": "recording 1: " + ENERGY_DEPTH % 64,
          "rate 0": "recording 0: the sample rate must be positive", "no samples": NO_SAMPLES, "length 2^31": "recording 0: 2^31 samples or more",
          "bad channels + bad depth": "recording 0: channels must be in [1, 16]", "bad depth + rate 0": "recording 0: " + ENERGY_DEPTH % 8,
          "x=None + bad table": NULL}
EVENTS_ALONE = {"filter=None": FILTER, "thr=None": FILTER, "hold=0": HOLD, "min_count=0": MIN_COUNT, "flags=2": FLAGS, "flags=-1": FLAGS,
                "n_classes=0": "n_classes must be in [1, 38400]", "n_classes=38401": "n_classes must be in [1, 38400]",
                "recording 65535": "row 3: recording must be in [0, 65534]", "recording -1": "row 0: recording must be in [0, 65534]",
                "window -1": "row 0: negative window", "class 4": "row 2: class_index outside the table", "class -1": "row 2: class_index outside the table",
                "window order": "row 2: rows must be nondecreasing in (recording, window)",
                "recording order": "row 2: rows must be nondecreasing in (recording, window)", "n=2^31": ROWS, "no=None": NULL, "o=None": NULL,
                "rows=None": NULL, "bad filter + n_classes=0": HOLD, "no=None + bad filter": NULL, "n=0 + bad filter": HOLD,
                "bad row + n_classes=0": "n_classes must be in [1, 38400]"}
WINDOWS = {"table=None": NULL, "first=None": NULL, "nr=0": RANGE, "nr=65536": RANGE, "clip=0": "n_samples must be positive", "hop=0": HOP,
           "hop=clip+1": HOP, "mt=-1": TAIL}
WINDOWS_FORM = {"plain": {"length 0": NO_SAMPLES, "2^36": BURST, "length 0 + bad hop": HOP, "first=None + bad hop": NULL},
                "mixed": {"bad depth + bad hop": "recording 0: " + DEPTH8, "first=None + bad table": NULL},
                "channels": {"bad depth + bad hop": "recording 0: " + DEPTH8, "bad channels + model_rate=0": "recording 0: channels must be in [1, 16]",
                             "first=None + bad table": NULL}}


def _arg(v):
    if isinstance(v, np.ndarray):
        return v.ctypes.data
    if isinstance(v, C.Structure):
        return C.addressof(v)
    return C.byref(v) if isinstance(v, C.c_size_t) else v


def _entry(lib, name, **defaults):
    """-> call(**broken): the entry with its well-formed arguments (in the C order) except the ones named; -> (code, text)."""
    f = getattr(lib, name)

    def call(**kw):
        assert set(kw) <= set(defaults), kw
        rc = f(*[_arg(v) for v in {**defaults, **kw}.values()])
        return int(rc), (lib.bnhip_last_error() or b"").decode()
    return call


def _stereo(bad, select=0):
    return host.channel_recordings(bad["length"], bad["rate"], bad["bits_per_sample"], 2, select)


def _check(got, want, where):
    """every case of `want` was run and answered E_INVALID with its text"""
    assert set(got) == set(want), (where, set(got) ^ set(want))
    for what, text in want.items():
        assert got[what] == (host.E_INVALID, text), (where, what, got[what])


def _analysis_entries(lib, m, n, keep):
    """{(form, answer): call} of the nine bnhip_analyze_*_pcm{_topk,,_events}, and the clips entry as ("channels", "clips")"""
    pcm = np.zeros(2 * n * 2 * 2, np.uint8)
    forms = {"plain": dict(h=m._h, x=pcm, bits=16, table=np.array([2 * n], np.int64), nr=1),
             "mixed": dict(h=m._h, x=pcm, table=host.recordings([2 * n], RATE, 16), nr=1, rate=RATE),
             "channels": dict(h=m._h, x=pcm, table=host.channel_recordings([2 * n], RATE, 16, 2, "mix"), nr=1, rate=RATE)}
    common = dict(hop=n // 2, mt=0, act=0, sens=1.0, k=5)
    thr = np.full(m.num_species(), 0.5, np.float32)
    keep["thr"] = thr
    answers = {"topk": dict(oc=np.zeros((8, 5), np.float32), oi=np.zeros((8, 5), np.int32)),
               "rows": dict(threshold=0.0, o=np.zeros(40, host.DETECTION), cap=40, no=C.c_size_t(0)),
               "events": dict(fs=host._EventFilterStruct(thr.ctypes.data, None, 0.5, 3, 1, 0), o=np.zeros(40, host.EVENT), cap=40, no=C.c_size_t(0))}
    suffix = {"topk": "_topk", "rows": "", "events": "_events"}
    prefix = {"plain": "bnhip_analyze_pcm", "mixed": "bnhip_analyze_mixed_pcm", "channels": "bnhip_analyze_channels_pcm"}
    out = {}
    for form, head in forms.items():
        for answer, tail in answers.items():
            extra = dict(chosen=np.zeros(4, np.int32)) if form == "channels" else {}
            out[form, answer] = _entry(lib, prefix[form] + suffix[answer], **head, **common, **tail, **extra)
    return out


def test_analysis_entries(built_lib, tiny_blob):
    lib = host._analyze_clips_protos(host.load_library())
    m = host.HipClassifier(tiny_blob, plan_only=True)
    multi = host.HipClassifier(tiny_blob, plan_only=True, devices=[0, 0])
    keep = {}
    try:
        n, nc = m.n_samples, m.num_species()
        thr = np.full(nc, 0.5, np.float32)
        flt = lambda thr=thr.ctypes.data, hold=3, min_count=1, flags=0: host._EventFilterStruct(thr, None, 0.5, hold, min_count, flags)
        k8 = min(nc, 8)
        long_one = n + (-(-(1 << 31) // k8) - 1)           # at hop 1: 2^31 / k8 windows (test_analyze_events_ref.py)
        for (form, answer), f in _analysis_entries(lib, m, n, keep).items():
            where = (form, answer)
            assert f() == (host.E_INVALID, PLAN_ONLY), where
            assert f(h=multi._h) == (host.E_INVALID, SINGLE), where
            got = {"h=None": f(h=None), "x=None": f(x=None), "table=None": f(table=None), "nr=0": f(nr=0), "nr=65536": f(nr=65536), "hop=0": f(hop=0),
                   "hop=n+1": f(hop=n + 1), "mt=-1": f(mt=-1), "k=0": f(k=0), "act=3": f(act=3)}
            _check(got, SHARED, where)
            if form == "plain":
                table = lambda length, bits=16: dict(table=np.array([length], np.int64), bits=bits)
                got = {"bits=8": f(bits=8), "bits=-16": f(bits=-16), "length 0": f(**table(0)), "bad depth + bad hop": f(bits=8, hop=0)}
            elif form == "mixed":
                table = lambda length, bits=16: dict(table=host.recordings([length], RATE, bits))
                got = {"bad depth + bad hop": f(**table(2 * n, 8), hop=0), "bad depth + model_rate=0": f(**table(2 * n, 8), rate=0)}
                _check({what: f(table=bad, nr=len(bad), rate=rate) for what, bad, rate in _bad_tables()}, BAD_TABLE, where)
            else:
                table = lambda length, bits=16, ch=2: dict(table=host.channel_recordings([length], RATE, bits, ch, "mix"))
                got = {"bad depth + bad hop": f(**table(2 * n, 8), hop=0), "bad channels + model_rate=0": f(**table(2 * n, 16, 17), rate=0)}
                _check({what: f(table=_stereo(bad, "mix"), nr=len(bad), rate=rate) for what, bad, rate in _bad_tables()}, BAD_TABLE, where)
                _check({what: f(table=bad, nr=len(bad)) for what, bad in _bad_channel_tables()}, BAD_CHANNELS, where)
            _check(got, FORM[form], where)
            if answer == "topk":
                got = {"oc=None": f(oc=None), "oi=None": f(oi=None)}
            elif answer == "rows":
                got = {"no=None": f(no=None), "o=None": f(o=None)}
            else:
                got = {"no=None": f(no=None), "o=None": f(o=None), "filter=None": f(fs=None), "thr=None": f(fs=flt(thr=None)), "hold=0": f(fs=flt(hold=0)),
                       "min_count=0": f(fs=flt(min_count=0)), "flags=2": f(fs=flt(flags=2)), "bad filter + k=0": f(fs=flt(hold=0), k=0),
                       "plan-only + 2^31 rows": f(**table(long_one), hop=1, k=k8, o=None, cap=0)}
            _check(got, ANSWER[answer], where)
    finally:
        m.close()
        multi.close()


def test_clips_entry(built_lib, tiny_blob):
    lib = host._analyze_clips_protos(host.load_library())
    m = host.HipClassifier(tiny_blob, plan_only=True)
    try:
        n, nc = m.n_samples, m.num_species()
        thr = np.full(nc, 0.5, np.float32)
        flt = lambda thr=thr.ctypes.data, hold=3, min_count=1, flags=0: host._EventFilterStruct(thr, None, 0.5, hold, min_count, flags)
        table = lambda length, bits=16, ch=2: host.channel_recordings([length], RATE, bits, ch, "mix")
        settings = lambda pre=100, post=200, most=1000, **kw: host.ClipSettings(pre, post, most, **kw)._struct()
        room = 40
        events, spans, loud = np.zeros(room, host.EVENT), np.zeros(room, host.CLIP_SPAN), (host.Loudness * room)()
        flac, off = np.zeros(1 << 16, np.uint8), np.zeros(room + 1, np.uint64)

        def out(events=events.ctypes.data, event_cap=room, spans=spans.ctypes.data, loudness=C.addressof(loud), offsets=off.ctypes.data):
            return host._ClipsOutStruct(events, event_cap, 0, spans, loudness, flac.ctypes.data, flac.size, offsets, None, 0, None, 0)

        f = _entry(lib, "bnhip_analyze_channels_pcm_clips", h=m._h, x=np.zeros(2 * n * 2 * 2, np.uint8), table=table(2 * n), nr=1, rate=RATE,
                   hop=n // 2, mt=0, act=0, sens=1.0, k=5, fs=flt(), chosen=np.zeros(4, np.int32), xs=settings(), out=out())
        assert f() == (host.E_INVALID, PLAN_ONLY)
        k8 = min(nc, 8)
        got = {"x=None": f(xs=None), "out=None": f(out=None), "spans=None": f(out=out(spans=None)), "flac_offsets=None": f(out=out(offsets=None)),
               "events=None": f(out=out(events=None)), "loudness=None": f(out=out(loudness=None)), "pre=-1": f(xs=settings(pre=-1)),
               "post=0": f(xs=settings(post=0)), "max=0": f(xs=settings(most=0)), "lpc=9": f(xs=settings(lpc_order=9)),
               "seek=-1": f(xs=settings(seek_interval=-1)), "rate=0": f(rate=0), "filter=None": f(fs=None), "thr=None": f(fs=flt(thr=None)),
               "hold=0": f(fs=flt(hold=0)), "min_count=0": f(fs=flt(min_count=0)), "flags=2": f(fs=flt(flags=2)),
               "flags=KEEP_DROPPED": f(fs=flt(flags=host.EVENTS_KEEP_DROPPED)), "bad filter + k=0": f(fs=flt(hold=0), k=0),
               "bad settings + bad filter": f(xs=settings(lpc_order=9), fs=flt(hold=0)),
               "bad channels + model_rate=0": f(table=table(2 * n, 16, 17), rate=0), "bad depth + bad hop": f(table=table(2 * n, 8), hop=0),
               "plan-only + 2^31 rows": f(table=table(n + (-(-(1 << 31) // k8) - 1)), hop=1, k=k8, out=out(events=None, event_cap=0))}
        _check(got, CLIPS, "clips")
        _check({"h=None": f(h=None), "x=None": f(x=None), "table=None": f(table=None)}, {w: NULL for w in ("h=None", "x=None", "table=None")}, "clips")
        _check({what: f(table=bad, nr=len(bad)) for what, bad in _bad_channel_tables()}, BAD_CHANNELS, "clips")
        _check({what: f(table=_stereo(bad, "mix"), nr=len(bad), rate=rate) for what, bad, rate in _bad_tables() if rate > 0},
               {w: t for w, t in BAD_TABLE.items() if t != RATE0}, "clips")
    finally:
        m.close()


def test_stand_alone_entries(built_lib):
    """bnhip_recording_clips_pcm16, bnhip_channel_energy_pcm, bnhip_detection_events: each only ever with an argument it refuses (a
    well-formed call would look for a device)."""
    lib = host._analyze_clips_protos(host.load_library())
    good = host.channel_recordings([1000, 500], [44100, RATE], [16, 24], [2, 3], ["auto", "mix"])
    pcm = np.zeros(1000 * 2 * 2 + 500 * 3 * 3, np.uint8)
    table = lambda bits=16, ch=2, rate=RATE, length=10: ch_recs([(rate, bits, length, ch, 0)])

    spans = np.zeros(2, host.CLIP_SPAN)
    spans["start"], spans["length"], spans["recording"] = [0, 100], [50, 60], [0, 1]

    def span(**kw):
        s = spans.copy()
        for field, v in kw.items():
            s[field][1] = v
        return s

    f = _entry(lib, "bnhip_recording_clips_pcm16", device=0, x=pcm, table=good, nr=2, rate=RATE, spans=spans, n_spans=2, out=np.zeros(128, np.int16))
    got = {"x=None": f(x=None), "spans=None": f(spans=None), "out=None": f(out=None), "rate=0": f(rate=0), "n_spans=0": f(n_spans=0),
           "n_spans=65536": f(n_spans=65536), "span recording=2": f(spans=span(recording=2)), "span recording=-1": f(spans=span(recording=-1)),
           "span length=-1": f(spans=span(length=-1)), "span start=-1": f(spans=span(start=-1)), "span past the end": f(spans=span(start=441)),
           "bad channels + model_rate=0": f(table=table(16, 17), nr=1, rate=0), "bad depth + bad span": f(table=table(8), nr=1, spans=span(length=-1)),
           "x=None + bad table": f(x=None, table=table(8), nr=1)}
    _check(got, SPANS, "recording_clips_pcm16")
    _check({what: f(table=bad, nr=len(bad)) for what, bad in _bad_channel_tables()}, BAD_CHANNELS, "recording_clips_pcm16")
    _check({what: f(table=_stereo(bad), nr=len(bad), rate=rate) for what, bad, rate in _bad_tables()}, BAD_TABLE, "recording_clips_pcm16")
    # the one refusal that is not an argument error yet needs no device: a rate whose phase table does not fit LDS (test_analyze_mixed.py)
    assert f(table=table(16, 2, 44100, 1000), nr=1, rate=256000, spans=span(recording=0), n_spans=1) == \
        (host.E_UNSUPPORTED, "recording 0: resampling 44100 Hz to 256000 Hz needs a phase table larger than LDS")

    e = _entry(lib, "bnhip_channel_energy_pcm", device=0, x=pcm, table=good, nr=2, o=np.zeros(64, host.CHANNEL_ENERGY), chosen=np.zeros(4, np.int32))
    got = {"x=None": e(x=None), "table=None": e(table=None), "o=None": e(o=None), "nr=0": e(nr=0), "nr=65536": e(nr=65536),
           "float32": e(table=table(0), nr=1), "depth 8": e(table=table(8), nr=1), "depth 64": e(table=ch_recs([(RATE, 16, 10, 2, 0), (RATE, 64, 10, 2, 0)])),
           "rate 0": e(table=table(rate=0), nr=1), "no samples": e(table=table(length=0), nr=1), "length 2^31": e(table=table(length=1 << 31), nr=1),
           "bad channels + bad depth": e(table=table(8, 17), nr=1), "bad depth + rate 0": e(table=table(8, rate=0), nr=1),
           "x=None + bad table": e(x=None, table=table(8), nr=1)}
    _check(got, ENERGY, "channel_energy_pcm")
    _check({what: e(table=bad, nr=len(bad)) for what, bad in _bad_channel_tables()},
           {**BAD_CHANNELS, "auto on float32": "recording 2: " + AUTO_FLOAT}, "channel_energy_pcm")

    rows = np.zeros(4, host.DETECTION)
    rows["window"], rows["class_index"], rows["confidence"] = [0, 1, 1, 2], [0, 1, 2, 3], 0.9
    thr = np.full(4, 0.5, np.float32)
    flt = lambda thr=thr.ctypes.data, hold=3, min_count=1, flags=0: host._EventFilterStruct(thr, None, 0.5, hold, min_count, flags)

    def edit(field, i, v):
        r = rows.copy()
        r[field][i] = v
        return r

    d = _entry(lib, "bnhip_detection_events", device=0, rows=rows, n=4, n_classes=4, fs=flt(), o=np.zeros(4, host.EVENT), cap=4, no=C.c_size_t(0))
    got = {"filter=None": d(fs=None), "thr=None": d(fs=flt(thr=None)), "hold=0": d(fs=flt(hold=0)), "min_count=0": d(fs=flt(min_count=0)),
           "flags=2": d(fs=flt(flags=2)), "flags=-1": d(fs=flt(flags=-1)), "n_classes=0": d(n_classes=0), "n_classes=38401": d(n_classes=38401),
           "recording 65535": d(rows=edit("recording", 3, 65535)), "recording -1": d(rows=edit("recording", 0, -1)),
           "window -1": d(rows=edit("window", 0, -1)), "class 4": d(rows=edit("class_index", 2, 4)), "class -1": d(rows=edit("class_index", 2, -1)),
           "window order": d(rows=edit("window", 2, 0)), "recording order": d(rows=edit("recording", 1, 1)), "n=2^31": d(n=1 << 31),
           "no=None": d(no=None), "o=None": d(o=None), "rows=None": d(rows=None), "bad filter + n_classes=0": d(fs=flt(hold=0), n_classes=0),
           "no=None + bad filter": d(no=None, fs=flt(hold=0)), "n=0 + bad filter": d(n=0, fs=flt(hold=0)),
           "bad row + n_classes=0": d(rows=edit("window", 0, -1), n_classes=0)}
    _check(got, EVENTS_ALONE, "detection_events")


def test_windows_entries(built_lib):
    lib = host._analyze_clips_protos(host.load_library())
    clip, hop = 24, 12
    first, n_out = np.zeros(64, np.int64), np.zeros(64, np.int64)
    forms = {"plain": _entry(lib, "bnhip_analyze_windows", table=np.array([100, 7], np.int64), nr=2, clip=clip, hop=hop, mt=0, first=first),
             "mixed": _entry(lib, "bnhip_analyze_mixed_windows", table=host.recordings([100, 7], RATE, 16), nr=2, rate=RATE, clip=clip, hop=hop, mt=0,
                             first=first, n_out=n_out),
             "channels": _entry(lib, "bnhip_analyze_channels_windows", table=host.channel_recordings([100, 7], RATE, 16, 2, 0), nr=2, rate=RATE,
                                clip=clip, hop=hop, mt=0, first=first, n_out=n_out)}
    for form, f in forms.items():
        assert f()[0] == 9, form
        got = {"table=None": f(table=None), "first=None": f(first=None), "nr=0": f(nr=0), "nr=65536": f(nr=65536), "clip=0": f(clip=0, hop=1),
               "hop=0": f(hop=0), "hop=clip+1": f(hop=clip + 1), "mt=-1": f(mt=-1)}
        _check(got, WINDOWS, form)
        if form == "plain":
            got = {"length 0": f(table=np.array([100, 0], np.int64)), "2^36": f(table=np.array([1 << 35, 1 << 35], np.int64)),
                   "length 0 + bad hop": f(table=np.array([100, 0], np.int64), hop=0), "first=None + bad hop": f(first=None, hop=0)}
        elif form == "mixed":
            got = {"bad depth + bad hop": f(table=host.recordings([100], RATE, 8), nr=1, hop=0),
                   "first=None + bad table": f(first=None, table=host.recordings([100], RATE, 8), nr=1)}
            _check({what: f(table=bad, nr=len(bad), rate=rate) for what, bad, rate in _bad_tables()}, BAD_TABLE, form)
        else:
            got = {"bad depth + bad hop": f(table=ch_recs([(RATE, 8, 100, 2, 0)]), nr=1, hop=0),
                   "bad channels + model_rate=0": f(table=ch_recs([(RATE, 16, 100, 17, 0)]), nr=1, rate=0),
                   "first=None + bad table": f(first=None, table=ch_recs([(RATE, 8, 100, 2, 0)]), nr=1)}
            _check({what: f(table=_stereo(bad), nr=len(bad), rate=rate) for what, bad, rate in _bad_tables()}, BAD_TABLE, form)
            _check({what: f(table=bad, nr=len(bad)) for what, bad in _bad_channel_tables()}, BAD_CHANNELS, form)
        _check(got, WINDOWS_FORM[form], form)
