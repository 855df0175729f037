"""The device FLAC decoder's frame reader (birdnet-go_amd/csrc/flac_parse.h) under AddressSanitizer + UBSan, in a stand-alone host
program (tests/native/flac_parse_main.cpp, plain g++, run as a child process) that walks a stream in the kernels' order: scan, parse,
link, restore.  It must reproduce tests/flaclpcdec.py's samples on every valid stream, and accept or reject a corpus of byte flips
and truncations without a finding; a flip inside frame j must be CORRUPT at frame j's start."""
import os
import struct
import subprocess

import numpy as np
import pytest

import flaccases
import flacdeccases as K
import flaclpccases
import flaclpcdec

HERE = os.path.dirname(os.path.abspath(__file__))
OK, BAD_METADATA, UNSUPPORTED, CORRUPT = 0, 1, 2, 3
STATUS = dict(OK=OK, BAD_METADATA=BAD_METADATA, UNSUPPORTED=UNSUPPORTED, CORRUPT=CORRUPT)


@pytest.fixture(scope="module")
def parse_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("asan") / "flac_parse_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", os.path.join(HERE, "native", "flac_parse_main.cpp"), "-o", out])
    return out


def _run(parse_bin, tmp_path, corpus):
    """-> per stream (status, frames, fail_offset, int16 samples)"""
    src, dst = tmp_path / "corpus.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        for b in corpus:
            f.write(struct.pack("<I", len(b)) + bytes(b))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([parse_bin, str(src), str(dst)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert int(r.stdout.split()[1]) == len(corpus)
    data, pos, out = dst.read_bytes(), 0, []
    for _ in corpus:
        status, frames, fail, n = struct.unpack_from("<iiQI", data, pos)
        pos += 20
        out.append((status, frames, fail, np.frombuffer(data, "<i2", n, pos)))
        pos += 2 * n
    assert pos == len(data)
    return out


def _first_stream(cases, name):
    blob, offsets, _, gained = cases.reference(name)
    return blob[:int(offsets[1])], np.asarray(gained[0], np.int16)


def test_valid_streams_decode_to_the_python_decoder_samples(parse_bin, tmp_path):
    corpus, want = [], []
    for name in K.FEATURE_NAMES:
        s, x, _ = K.feature(name)
        corpus.append(s)
        want.append(x)
    for cases, name in ((flaccases, "contents_one_clip"), (flaccases, "len1"), (flaccases, "len4097"), (flaclpccases, "contents_one_clip"),
                        (flaclpccases, "len17"), (flaclpccases, "contents_order1")):
        s, x = _first_stream(cases, name)
        corpus.append(s)
        want.append(x)
    s, x = K.off_chain()
    corpus.append(s)
    want.append(x)
    corpus.append(K.three_frames()[2])
    want.append(K.three_frames()[3])
    got = _run(parse_bin, tmp_path, corpus)
    for i, ((status, frames, fail, y), x) in enumerate(zip(got, want)):
        assert (status, fail) == (OK, 0), i
        assert y.size == x.size and np.array_equal(y, x), i


def test_damaged_streams_get_their_status_and_offset(parse_bin, tmp_path):
    d = K.damaged()
    got = _run(parse_bin, tmp_path, [v[0] for v in d.values()])
    for (name, (_, status, fail)), (gs, _, gf, y) in zip(d.items(), got):
        assert gs == STATUS[status] and y.size == 0, name
        assert gf == (fail or 0), name


def _seeds():
    seeds = [K.feature(n)[0] for n in ("bs192", "lpc32", "lpc1", "wasted1", "escapes", "rice_method1", "all_warmup", "last8")]
    seeds.append(_first_stream(flaccases, "contents_one_clip")[0])
    seeds.append(_first_stream(flaclpccases, "contents_one_clip")[0])
    return seeds


def test_mutated_streams_are_accepted_or_rejected_cleanly(parse_bin, tmp_path):
    rng = np.random.default_rng(919)
    corpus, expect = [], []                               # expect: None (anything clean), or the frame start a flip must be CORRUPT at
    for seed in _seeds():
        _, info = flaclpcdec.decode(seed)
        starts = [m["start"] for m in info["frames"]]
        corpus.append(seed)
        expect.append("intact")
        for _ in range(110):                              # one flip past the metadata: inside frame j
            at = int(rng.integers(starts[0], len(seed)))
            b = bytearray(seed)
            b[at] ^= int(rng.integers(1, 256))
            corpus.append(bytes(b))
            expect.append(max(s for s in starts if s <= at))
        for _ in range(25):                               # up to five flips anywhere, the metadata included
            b = bytearray(seed)
            for at in rng.integers(0, len(seed), int(rng.integers(1, 6))):
                b[at] ^= int(rng.integers(1, 256))
            corpus.append(bytes(b))
            expect.append(None)
        for cut in rng.integers(0, len(seed), 15):
            corpus.append(seed[:int(cut)])
            expect.append(None)
    got = _run(parse_bin, tmp_path, corpus)
    another_valid_stream = 0
    for (status, frames, fail, y), e in zip(got, expect):
        if e == "intact":
            assert status == OK
        elif e is not None:
            if status == OK:
                another_valid_stream += 1
            else:
                assert (status, fail) == (CORRUPT, e)
    assert another_valid_stream == 0
    assert len(corpus) == 10 * 151
