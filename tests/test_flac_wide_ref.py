"""The recording decoder without a GPU: the wide muxer (tests/flacwidemux.py) against the decoder restatement (tests/flacwidedec.py)
on every case; bnhip_flac_recording_info against the restatement's metadata, truncated at every byte, while bnhip_flac_stream_info
goes on answering UNSUPPORTED; and flac_parse.h's wide reader under AddressSanitizer + UBSan in a stand-alone host program
(tests/native/flac_parse_wide_main.cpp, plain g++, run as a child process, nothing preloaded) over every case, every damaged case
and a corpus of byte flips and truncations."""
import os
import struct
import subprocess

import numpy as np
import pytest

import flacwidecases as K
import flacwidedec as D
from birdnet_go_amd import host

HERE = os.path.dirname(os.path.abspath(__file__))
OK, BAD_METADATA, UNSUPPORTED, CORRUPT = 0, 1, 2, 3
STATUS = dict(OK=OK, BAD_METADATA=BAD_METADATA, UNSUPPORTED=UNSUPPORTED, CORRUPT=CORRUPT)


@pytest.mark.parametrize("name", list(K.cases()))
def test_muxer_and_restatement_round_trip(name):
    s, x, bits = K.cases()[name]
    y, info = D.decode(s)
    assert y.shape == x.shape and np.array_equal(y, x)
    assert (info["bits"], info["channels"], info["total"], info["rate"]) == (bits, x.shape[1], x.shape[0], K.RATE)


def test_round_trip_of_the_packing_burst_and_the_damaged_streams_are_refused():
    for s, x, _ in K.packing():
        assert np.array_equal(D.decode(s)[0], x)
    for name, v in K.damaged().items():
        with pytest.raises(D.WideFlacError):
            D.decode(v[0])


def test_the_cases_reach_what_they_are_named_for():
    c = K.cases()
    for bits in (16, 24):
        for assign, name in K.ASSIGN.items():
            frames = D.decode(c[f"{name}_{bits}"][0])[1]["frames"]
            assert {f["assign"] for f in frames} == {assign}
        kinds = D.decode(c[f"kinds_independent_{bits}"][0])[1]["frames"]
        for ch in (0, 1):
            seen = {(f["subframes"][ch]["kind"], f["subframes"][ch].get("order")) for f in kinds}
            assert {("CONSTANT", None), ("VERBATIM", None)} | {("FIXED", o) for o in range(5)} | {("LPC", o) for o in (1, 8, 9, 32)} <= seen
            assert {f["subframes"][ch].get("method") for f in kinds} >= {0, 1}
            coded = [f["subframes"][ch] for f in kinds if "porder" in f["subframes"][ch]]
            assert any(m["escapes"] == 1 and m["porder"] == 1 for m in coded)         # an escape partition beside a Rice one
            assert {m["porder"] for m in coded} >= {0, 1, 2, 3}
        for bs, tails in ((16, (1, 7)), (192, (1, 77)), (4096, (1, 333))):           # a short last frame of 1 and of an odd length
            for tail in tails:
                name = next(n for n in c if n.startswith(f"bs{bs}_") and n.endswith(f"_{bits}") and c[n][1].shape[0] % bs == tail)
                frames = D.decode(c[name][0])[1]["frames"]
                assert [f["block"] for f in frames] == [bs] * (len(frames) - 1) + [tail]
                assert all(m["porder"] == (2 if bs > 16 else 0) for f in frames[:-1] for m in f["subframes"])
        w =D.decode(c[f"wasted_{bits}"][0])[1]["frames"][0]["subframes"]
        assert (w[0]["wasted"], w[1]["wasted"]) == (2, 5)
        x = c[f"mid_side_odd_{bits}"][1]
        assert np.all((x[:, 0] + x[:, 1]) % 2 == 1)
        x = c[f"extremes_mid_side_{bits}"][1]
        assert int((x[:, 0] - x[:, 1]).max()) == (1 << bits) - 1
    # the 24-bit overflow case: one product is above 2^31, and the prediction sum (two coefficients' worth: the rest cancel) above 2^36
    x = c["lpc32_overflow_24"][1][:, 0]
    assert 16383 * int(np.abs(x).min()) > 2 ** 31 and 2 * 16383 * int(np.abs(x).min()) - 30 * 16383 * 200 > 2 ** 36
    # the same through the register window: order 8 at precision 15, in both channels
    s, x, _ = c["lpc8_overflow_24"]
    subs = [m for f in D.decode(s)[1]["frames"] for m in f["subframes"]]
    assert all((m["kind"], m["order"], m["precision"]) == ("LPC", 8, 15) for m in subs)
    assert 16383 * int(np.abs(x).min()) > 2 ** 31 and 2 * 16383 * int(np.abs(x).min()) - 6 * 16383 * 200 > 2 ** 36


def _fields(i):
    return dict(rate=i.rate, bits=i.bits, channels=i.channels, total=int(i.total_samples), block=i.max_block, min_block=i.min_block,
                min_frame=i.min_frame, max_frame=i.max_frame, audio=int(i.audio_offset), seek_points=i.seek_points)


@pytest.mark.parametrize("name", ["mid_side_24", "left_side_16", "mono_24", "mono_16", "cap_8192_24"])
def test_recording_info_against_the_restatement_truncated_at_every_byte(name):
    s = K.cases()[name][0]
    whole = D.metadata(s)
    for cut in range(whole["audio"] + 6):
        got = host.flac_recording_info(s[:cut])
        try:
            want = D.metadata(s[:cut])
        except D.WideFlacError:
            assert got.status == BAD_METADATA, cut
            continue
        assert got.status == OK and _fields(got) == want, cut
    assert host.flac_recording_info(s).status == OK


def test_stream_info_still_answers_unsupported_and_recording_info_refuses_what_is_out_of_scope():
    for name, (s, x, bits) in K.cases().items():
        clip = x.shape[1] == 1 and bits == 16
        assert host.flac_stream_info(s).status == (OK if clip else UNSUPPORTED), name
        assert host.flac_recording_info(s).status == OK, name
    assert host.flac_recording_info(K.above_cap()).status == UNSUPPORTED
    import flacmux
    s = K.cases()["mono_16"][0]
    for kw in (dict(channels=3), dict(bits=20), dict(bits=8), dict(bits=32), dict(bs=16385), dict(total=0), dict(min_block=16)):
        info = dict(bs=64, rate=K.RATE, total=300, min_frame=0, max_frame=0)
        info.update(kw)
        t = b"fLaC" + flacmux.block(0, flacmux.streaminfo(**info), last=True) + s[42:]
        assert host.flac_recording_info(t).status == UNSUPPORTED, kw
    t = bytearray(s)
    t[43] |= 1                                            # the first frame says variable block size
    assert host.flac_recording_info(bytes(t)).status == UNSUPPORTED


@pytest.fixture(scope="module")
def parse_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("asan") / "flac_parse_wide_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", os.path.join(HERE, "native", "flac_parse_wide_main.cpp"), "-o", out])
    return out


def _run(parse_bin, tmp_path, corpus):
    """-> per stream (status, frames, fail_offset, the PCM bytes)"""
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
        out.append((status, frames, fail, data[pos:pos + n]))
        pos += n
    assert pos == len(data)
    return out


def test_the_wide_reader_decodes_every_case_to_the_restatement_bytes(parse_bin, tmp_path):
    items = list(K.cases().items()) + [(f"packing{i}", v) for i, v in enumerate(K.packing())]
    got = _run(parse_bin, tmp_path, [v[0] for _, v in items])
    for (name, (s, x, bits)), (status, frames, fail, pcm) in zip(items, got):
        assert (status, fail) == (OK, 0), name
        assert frames == len(D.decode(s)[1]["frames"]), name
        assert pcm == D.pcm_bytes(x, bits), name


def test_the_wide_reader_on_every_damaged_case(parse_bin, tmp_path):
    d = K.damaged()
    got = _run(parse_bin, tmp_path, [v[0] for v in d.values()] + [K.above_cap()])
    for (name, (_, status, frames, fail, kept, bits)), (gs, gframes, gfail, pcm) in zip(d.items(), got):
        assert (gs, gframes, gfail) == (STATUS[status], frames, fail), name
        assert pcm == D.pcm_bytes(kept, bits), name
    assert got[-1][0] == UNSUPPORTED and got[-1][3] == b""


def test_mutated_recordings_are_accepted_or_rejected_cleanly(parse_bin, tmp_path):
    rng = np.random.default_rng(77)
    c = K.cases()
    corpus, expect = [], []
    for name in ("mid_side_24", "left_side_16", "kinds_independent_24", "kinds_side_right_16", "wasted_side_24", "lpc32_overflow_24",
                 "bs16_49_24", "verbatim_image_16"):
        seed = c[name][0]
        starts = [f["start"] for f in D.decode(seed)[1]["frames"]]
        for _ in range(60):                               # one flip inside frame j: CORRUPT at frame j's start
            at = int(rng.integers(starts[0], len(seed)))
            b = bytearray(seed)
            b[at] ^= int(rng.integers(1, 256))
            corpus.append(bytes(b))
            expect.append(max(s for s in starts if s <= at))
        for _ in range(15):                               # up to five flips anywhere, the metadata included
            b = bytearray(seed)
            for at in rng.integers(0, len(seed), int(rng.integers(1, 6))):
                b[at] ^= int(rng.integers(1, 256))
            corpus.append(bytes(b))
            expect.append(None)
        for cut in rng.integers(0, len(seed), 10):
            corpus.append(seed[:int(cut)])
            expect.append(None)
    got = _run(parse_bin, tmp_path, corpus)
    for (status, frames, fail, pcm), e in zip(got, expect):
        if e is not None:
            assert (status, fail) == (CORRUPT, e)
