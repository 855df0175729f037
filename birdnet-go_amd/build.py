"""Build driver: compiles the HIP/C++ engine for gfx950 into lib/libbnhip.so (in-tree, so the
built library travels with the repo snapshot to the GPU box)."""
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.environ.get("BNHIP_LIBDIR") or os.path.join(HERE, "lib")      # (BNHIP_LIBDIR + BNHIP_EXTRA_FLAGS: an A/B build beside the shipped one)
LIB = os.path.join(LIBDIR, "libbnhip.so")
SOURCES = ["frontend.hip", "conv.hip", "pw_gemm.hip", "pw_bx3.hip", "dwconv.hip", "post.hip", "expdw.hip", "pw_b16.hip", "pw_ws.hip", "generic.hip", "resample.hip", "eq.hip", "soundlevel.hip", "heatmap.hip", "stft.hip", "spectrogram.hip", "loudness.hip", "flac.hip", "flac_decode.hip", "png.hip", "denoise.hip", "analyze.hip", "channels.hip", "engine.cpp", "tune.cpp", "planner.cpp", "graph_passes.cpp", "tflite_model.cpp", "model_onnx.cpp", "hostpipe.cpp", "numa.cpp", "windows.cpp", "api.cpp", "api_windows.cpp", "api_model.cpp", "api_predict.cpp", "api_ultrasonic.cpp", "api_resample.cpp", "api_eq.cpp", "api_soundlevel.cpp", "api_spectrogram.cpp", "api_loudness.cpp", "api_flac.cpp", "api_flac_decode.cpp", "api_png.cpp", "api_denoise.cpp", "api_analyze.cpp", "events.hip", "clips.hip", "api_clips.cpp", "analyze_recordings.cpp", "api_events.cpp", "api_channels.cpp", "events_bank.hip", "api_event_bank.cpp", "capture_bank.hip", "api_capture_bank.cpp", "levels.hip", "api_level.cpp"]
# (a new unit goes last, as events.hip, then events_bank.hip / api_event_bank.cpp then capture_bank.hip / api_capture_bank.cpp and then levels.hip / api_level.cpp did: units linked behind a new one move, and the headline benchmark was 0.2 % slower with events.hip mid-list - DESIGN section 9)
HEADERS = ["kernels.h", "pw_common.h", "engine.h", "tflite_model.h", "model_onnx.h", "hostpipe.h", "numa.h", "windows.h", "resample.h", "eq_bank.h", "soundlevel_bank.h", "heatmap.h", "spectrogram.h", "loudness.h", "pcmgain.h", "flac.h", "flac_decode.h", "flac_parse.h", "png.h", "block_scan.h", "ragged.h", "pcm_sample.h", "fft_r8.h", "fft_passes.h", "denoise.h", "process_chain.h", "analyze.h", "channels.h", "events.h", "clips.h", "clip_source.h", "analyze_recordings.h", "api_events.h", "events_bank.h", "capture_bank.h", "levels.h", "api_common.h", "api_oneshot.h", "api_model.h", "stream_bank.h", os.path.join("..", "..", "include", "bnhip.h")]
# -fno-slp-vectorize: gfx950 hazard, reproduced standalone (tools/ubench/pkf32_vs_bf16mfma.hip, profiles/r04_pk_hazard.txt): a
# packed-fp32 VALU instruction whose op_sel bit for src1 is set (v_pk_fma_f32 / v_pk_mul_f32 ... op_sel:[0,1,..]: the LOW result
# computed from src1's HIGH half) returns a wrong low half in lanes 48-63 while another wave on the same CU executes
# v_mfma_f32_16x16x32_bf16 - i.e. whenever the other pipeline context runs a split-bf16 GEMM.  The SLP vectoriser forms exactly
# these when it packs two scalar fmaf chains that share a broadcast operand (176 of them in stft.hip: 2-4 % of clips wrong with
# two contexts in flight).  tests/test_isa_audit.py disassembles the built library and fails on any such instruction.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-unused-value", "-ffp-contract=off", "-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form"]
FLAGS += os.environ.get("BNHIP_EXTRA_FLAGS", "").split()
NO_VGPR_FORM = set()     # sources to compile without the VGPR-form MFMA rewrite (none at present)


def _digest():
    h = hashlib.sha256()
    for f in SOURCES + HEADERS:
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(fh.read())
    h.update(" ".join(FLAGS).encode())
    return h.hexdigest()


def build(force=False, verbose=False):
    os.makedirs(LIBDIR, exist_ok=True)
    stamp = os.path.join(LIBDIR, ".build_digest")
    dig = _digest()
    if not force and os.path.exists(LIB) and os.path.exists(stamp) and open(stamp).read() == dig:
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # per-object stamps: a translation unit is recompiled only when it, a header or the flags changed
    hh = hashlib.sha256()
    for f in HEADERS:
        with open(os.path.join(CSRC, f), "rb") as fh:
            hh.update(fh.read())
    hh.update(" ".join(FLAGS).encode())
    objs, cmds = [], []
    for src in SOURCES:
        obj = os.path.join(LIBDIR, os.path.splitext(src)[0] + ".o")
        objs.append(obj)
        h = hh.copy()
        with open(os.path.join(CSRC, src), "rb") as fh:
            h.update(fh.read())
        ostamp, odig = obj + ".digest", h.hexdigest()
        if not force and os.path.exists(obj) and os.path.exists(ostamp) and open(ostamp).read() == odig:
            continue
        flags = [f for f in FLAGS if src not in NO_VGPR_FORM or f not in ("-mllvm", "-amdgpu-mfma-vgpr-form")]
        cmds.append(([hipcc, "-x", "hip"] + flags + ["-c", os.path.join(CSRC, src), "-o", obj], ostamp, odig))
    # the translation units are independent: compile them side by side
    procs = []
    for cmd, ostamp, odig in cmds:
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        if os.path.exists(ostamp):
            os.remove(ostamp)
        procs.append((cmd, ostamp, odig, subprocess.Popen(cmd)))
    failed = None
    for cmd, ostamp, odig, pr in procs:
        if pr.wait() != 0:
            failed = failed or (pr.returncode, cmd)
        else:
            with open(ostamp, "w") as fh:
                fh.write(odig)
    if failed:
        raise subprocess.CalledProcessError(*failed)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
    subprocess.check_call(cmd)
    with open(stamp, "w") as fh:
        fh.write(dig)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
