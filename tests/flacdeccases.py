"""The streams of the FLAC decoder's tests, shared by the CPU tests (test_flac_decode_ref.py, test_flac_decode_asan.py) and the device
tests (test_flac_decode.py): feature streams written by tests/flacmux.py, one feature each and 2-3 frames long, and the damaged
streams of the mixed burst.  Every stream is built once and never changed; the expected samples come from tests/flaclpcdec.py."""
import functools

import numpy as np

import flaclpcdec
import flacmux


def _rng(seed):
    return np.random.default_rng(seed)


def _noise(seed, n, amp):
    return _rng(seed).integers(-amp, amp + 1, n)


def _lpc32():
    coefs = [int(v) for v in _rng(5).integers(-(1 << 14), 1 << 14, 32)]
    return dict(kind="LPC", order=32, coefs=coefs, precision=15, shift=15, method=1, porder=1)


def _loud_quiet(bs, parts, loud, amp, seed):
    """zeros, with +-amp noise in the partitions listed in `loud`"""
    x = np.zeros(bs, np.int64)
    n = bs // parts
    for p in loud:
        x[p * n:(p + 1) * n] = _noise(seed + p, n, amp)
    return x


def _rice_method1():
    # partitions 1..15 carry Rice parameters 16..30 (17 to 31 bits a sample), the other 17 zeros at one bit a sample: the frame stays
    # below the VERBATIM bound
    x = np.concatenate([_loud_quiet(4096, 32, range(1, 16), 30000, 40), _loud_quiet(4096, 32, range(1, 16), 30000, 80)])
    ks = [0] + list(range(16, 31)) + [0] * 16
    return flacmux.stream(x, 4096, 48000, dict(kind="FIXED", order=0, method=1, porder=5, ks=ks))


def _escapes():
    x = np.concatenate([np.zeros(64), _noise(1, 64, 0) + _rng(2).integers(-1, 1, 64), _noise(3, 64, 30000), _noise(4, 64, 200)] * 2 + [np.zeros(64)])
    spec = dict(kind="FIXED", order=0, porder=2, ks=[("esc", 0), ("esc", 1), ("esc", 16), None])
    last = dict(kind="FIXED", order=0, porder=0, ks=[("esc", 0)])
    return flacmux.stream(x.astype(np.int64), 256, 44100, [spec, spec, last])


def _features():
    f = {}
    for bs in (16, 192, 576, 4608, 16384):
        spec = dict(kind="FIXED", order=1, porder=2)
        f[f"bs{bs}"] = lambda bs=bs, spec=spec: flacmux.stream(np.cumsum(_noise(bs, 2 * bs + bs // 3 + 1, 20)), bs, 48000, [spec, spec, dict(spec, porder=0)])
    f["last8"] = lambda: flacmux.stream(_noise(11, 2 * 4096 + 200, 3000), 4096, 48000, [dict(kind="FIXED", order=2)] * 2 + [dict(kind="FIXED", order=0, bs_form=8)])
    f["last16"] = lambda: flacmux.stream(_noise(12, 2 * 4096 + 1000, 3000), 4096, 48000, [dict(kind="FIXED", order=2)] * 2 + [dict(kind="FIXED", order=3, bs_form=16)])
    f["rate12"] = lambda: flacmux.stream(_noise(13, 1152 * 2 + 5, 900), 1152, 250000, dict(kind="FIXED", order=1, rate_form=12))
    f["rate13"] = lambda: flacmux.stream(_noise(14, 1152 * 2 + 5, 900), 1152, 11025, dict(kind="FIXED", order=1, rate_form=13))
    f["rate14"] = lambda: flacmux.stream(_noise(15, 1152 * 2 + 5, 900), 1152, 384000, dict(kind="FIXED", order=1, rate_form=14))
    f["lpc32"] = lambda: flacmux.stream(_noise(16, 2 * 1024 + 77, 20), 1024, 48000, [_lpc32(), _lpc32(), dict(_lpc32(), porder=0)])
    f["lpc1"] = lambda: flacmux.stream(np.cumsum(_noise(17, 2 * 512 + 9, 25)), 512, 32000, dict(kind="LPC", order=1, coefs=[-1], precision=1, shift=0))
    f["wasted1"] = lambda: flacmux.stream(2 * _noise(18, 2 * 256 + 40, 9000), 256, 48000, dict(kind="FIXED", order=2, wasted=1))
    f["wasted15"] = lambda: flacmux.stream(-32768 * _rng(19).integers(0, 2, 3 * 256), 256, 48000,
                                           [dict(kind="VERBATIM", wasted=15), dict(kind="FIXED", order=1, wasted=15), dict(kind="FIXED", order=0, wasted=15)])
    f["constant_wasted"] = lambda: flacmux.stream(np.full(2 * 256 + 3, -4096), 256, 48000, dict(kind="CONSTANT", wasted=12))
    f["rice_method1"] = _rice_method1
    f["escapes"] = _escapes
    f["porder8"] = lambda: flacmux.stream(np.cumsum(_noise(20, 2 * 4096, 20)) * np.repeat(np.resize([1, 3, 0, 2], 512), 16), 4096, 48000,
                                          dict(kind="FIXED", order=2, porder=8))
    f["all_warmup"] = lambda: flacmux.stream(_noise(21, 3 * 16, 30000), 16, 48000,
                                             dict(kind="LPC", order=16, coefs=list(range(-8, 8)), precision=5, shift=2, bs_form=8))
    f["number7"] = lambda: flacmux.stream(_noise(22, 2 * 192 + 1, 100), 192, 48000, [dict(kind="FIXED", order=1, number_bytes=n) for n in (7, 4, 2)])
    f["metadata_blocks"] = lambda: flacmux.stream(_noise(23, 2 * 192, 100), 192, 48000, blocks=[(1, bytes(37)), (4, b"\x04\0\0\0test\0\0\0\0"), (3, bytes(16) + (192).to_bytes(2, "big"))])
    return f


_FEATURES = _features()
FEATURE_NAMES = tuple(_FEATURES)


@functools.lru_cache(maxsize=None)
def feature(name):
    """-> (stream bytes, the samples flaclpcdec decodes from it as int16, flaclpcdec's info)"""
    s = _FEATURES[name]()
    x, info = flaclpcdec.decode(s)
    return s, x.astype(np.int16), info


@functools.lru_cache(maxsize=None)
def three_frames():
    """The intact stream the damaged ones are made from: 3 frames of 576 -> (head, [frame bytes], stream, samples, info)"""
    x = _noise(30, 2 * 576 + 100, 5000)
    head, frames = flacmux.stream(x, 576, 48000, dict(kind="FIXED", order=2, porder=1), parts=True)
    s = head + b"".join(frames)
    y, info = flaclpcdec.decode(s)
    return head, frames, s, y.astype(np.int16), info


def _flip(s, at, bit=0x10):
    b = bytearray(s)
    b[at] ^= bit
    return bytes(b)


@functools.lru_cache(maxsize=None)
def damaged():
    """name -> (stream, expected status name, expected fail_offset or None where the metadata is refused)"""
    head, frames, s, _, info = three_frames()
    st = [m["start"] for m in info["frames"]]
    x = _noise(30, 2 * 576 + 100, 5000)
    d = {}
    d["crc16_flip"] = (_flip(s, st[1] + len(frames[1]) // 2), "CORRUPT", st[1])
    d["crc8_flip"] = (_flip(s, st[2] + 2, 0x01), "CORRUPT", st[2])
    d["truncated"] = (s[:-7], "CORRUPT", st[2])
    d["trailing"] = (s + b"\x00\xff\xf8garbage", "CORRUPT", len(s))
    d["missing_frame"] = (head + frames[0] + frames[2], "CORRUPT", st[1])
    d["stereo"] = (flacmux.stream(x, 576, 48000, info=dict(channels=2)), "UNSUPPORTED", None)
    d["bits24"] = (flacmux.stream(x, 576, 48000, info=dict(bits=24)), "UNSUPPORTED", None)
    d["variable"] = (flacmux.stream(x, 576, 48000, dict(kind="FIXED", order=2, variable=True)), "UNSUPPORTED", None)
    d["total0"] = (flacmux.stream(x, 576, 48000, info=dict(total=0)), "UNSUPPORTED", None)
    # FIXED order 1 from a warm-up of 32767 and a residual of +1000: the second sample is 33767
    over = [32767, 33767] + [33767] * 574
    h2, f2 = flacmux.stream(np.concatenate([x[:576], over, x[:50]]), 576, 48000,
                            [dict(kind="FIXED", order=2), dict(kind="FIXED", order=1), dict(kind="FIXED", order=0)], parts=True)
    d["overflow"] = (h2 + b"".join(f2), "CORRUPT", len(h2) + len(f2[0]))
    return d


@functools.lru_cache(maxsize=None)
def off_chain():
    """A stream whose first frame is VERBATIM and whose samples are, byte for byte, a complete valid image of frame 2 (its number, its
    block size, both CRCs right): a candidate the chain never reaches.  -> (stream, flaclpcdec's samples as int16)"""
    bs = 192
    tail = _noise(31, 70, 3000)                      # frame 2: the short last frame
    real = flacmux.frame([int(v) for v in tail], 2, 48000, dict(kind="FIXED", order=1))
    image = real + bytes((-len(real)) % 2)
    payload = np.frombuffer(image, ">i2").astype(np.int64)
    first = np.concatenate([_noise(32, 5, 100), payload, _noise(33, bs, 100)])[:bs]
    assert 5 + payload.size <= bs
    x = np.concatenate([first, _noise(34, bs, 3000), tail])
    s = flacmux.stream(x, bs, 48000, [dict(kind="VERBATIM"), dict(kind="FIXED", order=2), dict(kind="FIXED", order=1)])
    assert s.count(real) == 2
    y, _ = flaclpcdec.decode(s)
    return s, y.astype(np.int16)
