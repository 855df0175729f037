"""Parity at the headline configuration and on the reference's own audio fixture (VERDICT r1 "Next" #1).

* BASELINE configs[1] at its own size: batch 256 through the depth-2 engine the bench uses, sampled rows vs the oracle.
* tawnyowl.wav (the reference's sample file): five 3 s clips through the 32-bit PCM entry vs the oracle.
* The real-artefact harness: with BNHIP_REAL_MODEL (+ BNHIP_REAL_CLIPS_F32 / BNHIP_REAL_LABEL) set, the real `.tflite` is
  planned and run; shape cloned from the reference's own cross-backend parity test
  (internal/inference/openvino_parity_functional_test.go:56,112-116,366-382: top-1 identical, |sigma(a)-sigma(b)| <= 0.05).
  Without the environment it skips cleanly - the day the weights appear, nothing needs writing.
"""
import os

import numpy as np
import pytest

from birdnet_go_amd import host, synth_model as sm
from oracle import gofuncs as G
from oracle.interp import Interpreter

from test_parity_gpu import PROB_TOL, _DevBuf, assert_parity, sig

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TAWNY_LABEL = 5760            # `Strix aluco_Tawny Owl`: data/labels/V2.4/BirdNET_GLOBAL_6K_V2.4_Labels_en_uk.txt:5761 (0-based 5760)


def tawnyowl_pcm32():
    z = np.load(os.path.join(GOLD, "tawnyowl_pcm32.npz"))
    acc = np.cumsum(z["delta"].astype(np.int64))
    return ((acc + 2**31) % 2**32 - 2**31).astype("<i4")


def test_tawnyowl_fixture_is_intact():
    """CPU: the committed fixture decodes to the 720 000 PCM words of the reference's tawnyowl.wav (sha256 recorded when
    tests/golden/make_tawnyowl.py ran against the reference's file), the file rebuilt from the fixtures reads back through
    wav.read_wav as the Go-restated conversion of those words, and it frames into five 3 s clips."""
    import hashlib
    from birdnet_go_amd import wav
    from test_wav import tawnyowl_wav_bytes
    pcm = tawnyowl_pcm32()
    z = np.load(os.path.join(GOLD, "tawnyowl_pcm32.npz"))
    assert pcm.size == 720000 and hashlib.sha256(pcm.tobytes()).digest() == z["sha256"].tobytes()
    s, rate, bits = wav.read_wav(tawnyowl_wav_bytes())
    assert (rate, bits) == (48000, 32) and np.array_equal(s, G.pcm_to_f32(pcm.tobytes(), 32))
    clips, starts = wav.frame_clips(G.pcm_to_f32(pcm.tobytes(), 32), 48000)
    assert clips.shape == (5, 144000) and list(starts) == [0.0, 3.0, 6.0, 9.0, 12.0]


@pytest.mark.gpu
def test_tawnyowl_five_clips_pcm32_vs_oracle(gpu, full_blob):
    """BASELINE configs[0] input: tawnyowl.wav -> five clips -> 32-bit PCM entry (device-side /2147483648) -> engine, vs the
    oracle fed the Go-restated conversion of the same bytes; also through wav.analyze_file-style framing + device top-k."""
    pcm = tawnyowl_pcm32()
    x = G.pcm_to_f32(pcm.tobytes(), 32).reshape(5, 144000)
    ref = Interpreter(full_blob).invoke(x)[0]
    clf = host.HipClassifier(full_blob, max_batch=8)
    try:
        got = clf.predict_pcm(pcm.tobytes(), 32, 5)
        assert_parity(got, ref)
        assert np.abs(got - ref).max() < 1e-3
        conf, idx = clf.predict_topk(x.reshape(-1), 5, k=10, sensitivity=1.0)
        want = G.sigmoid_sensitivity(ref, 1.0)
        assert (idx[:, 0] == ref.argmax(1)).all()
        assert np.abs(conf[:, 0] - want.max(1)).max() <= PROB_TOL
    finally:
        clf.close()


@pytest.mark.gpu
def test_batch256_depth2_sampled_rows_vs_oracle(gpu, full_blob):
    """The configuration the bench line is quoted on, checked at its own size: 256 config-2 clips through the depth-2 engine
    (full-batch tiles chosen by padded work, two contexts in flight), rows {0, 63, 127, 128, 255} vs the oracle.  Round 1's
    k_pw_gemm staging overflow produced logits off by 2.0 exactly here while every smaller parity test stayed green."""
    B = 256
    xh = sm.synth_clips(B, 144000, 48000)
    rows = [0, 63, 127, 128, 255]
    ref = Interpreter(full_blob).invoke(xh[rows])[0]
    clf = host.HipClassifier(full_blob, max_batch=B, depth=2, lanes=1)
    x, out = _DevBuf(xh.nbytes), _DevBuf(2 * B * 6522 * 4)
    try:
        x.upload(xh)
        for i in range(3):                                          # three calls in flight over the two contexts
            clf.predict_device(x.at(0), B, out.at((i & 1) * B * 6522 * 4))
        clf.synchronize()
        o0 = out.download((2, B, 6522))
        assert np.array_equal(o0[0], o0[1])                         # both contexts compute the same thing, bit for bit
        got = o0[0][rows]
        assert_parity(got, ref)
        assert np.abs(got - ref).max() < 1e-3
        # and the same rows through the host-pointer entry of a default engine (two lanes, split H2D)
        d = host.HipClassifier(full_blob, max_batch=B)
        try:
            h = d.predict_batch(xh.reshape(-1), B)
            assert np.abs(h - o0[0]).max() < 1e-4
            assert_parity(h[rows], ref)
        finally:
            d.close()
    finally:
        clf.close(); x.free(); out.free()


@pytest.mark.gpu
def test_batch1024_depth2_sampled_rows_vs_oracle(gpu, full_blob):
    """BASELINE configs[2] at its per-GPU shard size (8 192 clips over 8 GPUs = 1 024 per GPU): `max_batch` 1 024, depth 2, inputs
    resident in HBM, three calls in flight over the two contexts; rows {0, 511, 512, 1023} vs the oracle, both contexts
    bit-identical, the last 256 clips against what a 256-clip engine computes for them (its own tiles: summation-order
    tolerance) - then the same 1 024 clips through the blocking host-pointer entry of a default engine.
    VERDICT r5 item 1: round 1's logits-off-by-2.0 bug lived exactly in "only at full size", and nothing ran at 1 024."""
    B = 1024
    xh = sm.synth_clips(B, 144000, 48000)
    rows = [0, 511, 512, 1023]
    ref = Interpreter(full_blob).invoke(xh[rows])[0]
    clf = host.HipClassifier(full_blob, max_batch=B, depth=2, lanes=1)
    x, out = _DevBuf(xh.nbytes), _DevBuf(2 * B * 6522 * 4)
    try:
        x.upload(xh)
        for i in range(3):
            clf.predict_device(x.at(0), B, out.at((i & 1) * B * 6522 * 4))
        clf.synchronize()
        o0 = out.download((2, B, 6522))
        assert np.isfinite(o0).all()
        assert np.array_equal(o0[0], o0[1])
        got = o0[0][rows]
        assert_parity(got, ref)
        assert np.abs(got - ref).max() < 1e-3
        # the last 256 clips through a 256-clip engine (other tiles, other grid fill): within the summation-order tolerance
        c256 = host.HipClassifier(full_blob, max_batch=256, depth=2, lanes=1)
        try:
            o256 = _DevBuf(256 * 6522 * 4)
            c256.predict_device(x.at(768 * 144000 * 4), 256, o256.at(0))
            c256.synchronize()
            assert np.abs(o256.download((256, 6522)) - o0[0][768:]).max() < 1e-4
            o256.free()
        finally:
            c256.close()
    finally:
        clf.close(); x.free(); out.free()
    d = host.HipClassifier(full_blob, max_batch=B)
    try:
        h = d.predict_batch(xh.reshape(-1), B)
        assert np.abs(h - o0[0]).max() < 1e-4
        assert_parity(h[rows], ref)
    finally:
        d.close()


def _softmax64(v):
    z = np.asarray(v, np.float64)
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


@pytest.mark.gpu
@pytest.mark.parametrize("prec,tol", [("f32", 1e-4), ("bf16", 2e-2)])
def test_perch_batch512_depth2_sampled_rows_vs_oracle(gpu, prec, tol):
    """BASELINE configs[4] at its per-GPU shard size (4 096 clips over 8 GPUs = 512 per GPU), fp32 and bf16 engines: 512 clips of
    5 s @ 32 kHz resident in HBM, depth 2, three calls in flight; rows {0, 255, 256, 511}: softmax vs the fp32 oracle (1e-4 fp32;
    2e-2 bf16 - the reference accepts 0.08 on an f16 GPU, openvino_parity_functional_test.go:156-158), top-1 identical, the 1536-d
    embedding output too (2e-3 relative fp32, the reference's own cross-runtime expectation model_openvino.go:263-265; 5e-2 bf16),
    both contexts bit-identical."""
    cfg = sm.perch_config()
    blob = sm.build_model(cfg)
    B = 512
    xh = sm.synth_clips(B, cfg.n_samples, cfg.sample_rate)
    rows = [0, 255, 256, 511]
    outs = Interpreter(blob).invoke(xh[rows])
    ref, ref_emb = outs[3], outs[0]
    clf = host.HipClassifier(blob, max_batch=B, depth=2, lanes=1, precision=prec)
    nc, ed = clf.num_species(), clf.emb_dim
    assert (nc, ed) == (14795, 1536)
    x, out, emb = _DevBuf(xh.nbytes), _DevBuf(2 * B * nc * 4), _DevBuf(2 * B * ed * 4)
    try:
        x.upload(xh)
        for i in range(3):
            clf.predict_device(x.at(0), B, out.at((i & 1) * B * nc * 4), emb.at((i & 1) * B * ed * 4))
        clf.synchronize()
        o, e = out.download((2, B, nc)), emb.download((2, B, ed))
        assert np.isfinite(o).all() and np.isfinite(e).all()
        assert np.array_equal(o[0], o[1]) and np.array_equal(e[0], e[1])
        got = o[0][rows]
        assert (got.argmax(1) == ref.argmax(1)).all()
        d = float(np.abs(_softmax64(got) - _softmax64(ref)).max())
        assert d <= tol, d
        scale = float(np.abs(ref_emb).max())
        de = float(np.abs(e[0][rows] - ref_emb).max()) / scale
        assert de <= (2e-3 if prec == "f32" else 5e-2), de
    finally:
        clf.close(); x.free(); out.free(); emb.free()


# ------------------------------------------------------------------------------------------------ real artefacts (env-gated)
REAL_MODEL = os.environ.get("BNHIP_REAL_MODEL")


@pytest.mark.gpu
@pytest.mark.skipif(not REAL_MODEL, reason="BNHIP_REAL_MODEL not set (real BirdNET .tflite is absent from the reference snapshot)")
def test_real_model_tawnyowl_top1_and_clips(gpu):
    """BNHIP_REAL_MODEL=/path/BirdNET_GLOBAL_6K_V2.4_Model_FP32.tflite
       BNHIP_REAL_CLIPS_F32=/path/clips.f32        optional: float32 [n, 144000] clips (the reference harness' format)
       BNHIP_REAL_EXPECTED_F32=/path/logits.f32    optional: float32 [n, classes] logits of the TFLite CPU path on those clips
       BNHIP_REAL_LABEL=5760                       optional: expected top-1 on every tawnyowl clip (default 5760)
    Plans the real graph (any unsupported operator is reported by name), asserts top-1 on tawnyowl, prints max |d sigma|
    vs the oracle and, when TFLite's own logits are supplied, applies the reference's gate to them."""
    blob = open(REAL_MODEL, "rb").read()
    clf = host.HipClassifier(blob, max_batch=8)
    try:
        pcm = tawnyowl_pcm32()
        x = G.pcm_to_f32(pcm.tobytes(), 32).reshape(5, -1)
        assert x.shape[1] == clf.n_samples, f"model takes {clf.n_samples} samples"
        got = clf.predict_pcm(pcm.tobytes(), 32, 5)
        want_label = int(os.environ.get("BNHIP_REAL_LABEL", TAWNY_LABEL))
        top = got.argmax(1)
        print("tawnyowl top-1 per clip:", top.tolist(), "confidence", sig(got.max(1)).round(4).tolist())
        assert (np.bincount(top).argmax() == want_label), f"majority top-1 {np.bincount(top).argmax()} != {want_label}"
        ref = Interpreter(blob).invoke(x[:2])[0]
        d = float(np.abs(sig(got[:2]) - sig(ref)).max())
        print(f"max |d sigma| vs oracle on 2 clips: {d:.3e}")
        assert (got[:2].argmax(1) == ref.argmax(1)).all() and d <= PROB_TOL
        clips = os.environ.get("BNHIP_REAL_CLIPS_F32")
        if clips:
            xc = np.fromfile(clips, np.float32).reshape(-1, clf.n_samples)
            gc = clf.predict_batch(xc.reshape(-1), xc.shape[0])
            exp = os.environ.get("BNHIP_REAL_EXPECTED_F32")
            if exp:
                e = np.fromfile(exp, np.float32).reshape(xc.shape[0], -1)
                dd = float(np.abs(sig(gc) - sig(e)).max())
                print(f"max |d sigma| vs TFLite on {xc.shape[0]} clips: {dd:.3e}")
                assert (gc.argmax(1) == e.argmax(1)).all() and dd <= 0.05       # openvino_parity_functional_test.go:56,112-116
    finally:
        clf.close()
