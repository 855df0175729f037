"""Full-width form of k_expand_dw (csrc/expdw.hip): tools/ubench/expdw_fullw_check drives
launch_expand_dw with an explicit shape index over the smallest layers at which the in-image column mapping can go wrong - 6 x 32,
5 x 32, 3 x 32 and their transposes on the three tile shapes of the 6 x 32 layers, Cin 40 / 48 / 112, Cmid 36 / 96, f32 and
split-bf16 phase 1, with and without a sums buffer - and over the neighbours (W = 31, 33, 64) that must keep the footprint mapping.

The form is a pure re-mapping of which GEMM row computes which pixel: the program runs twice, as separate processes - defaults and
BNHIP_EXPDW_FULLW=0 - and every output tensor and every per-tile sum must come out bit-identical.  (The role rotation that was to be the
third run was not built: wave i lands on no fixed SIMD - profiles/r10_wave_placement.txt)  Each run is also held to the fp64 loop nest by the gate of
tests/test_expdw_lab.py: error <= 4 x the error of a plain fp32 evaluation + 2^-22 (in units of the output scale).  Without a GPU: the case list reports the full-width form for each eligible case and for no neighbour."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ({}, {"BNHIP_EXPDW_FULLW": "0"})
CASE = re.compile(r"^CASE (\S+) eligible=(\d) fullw=(\d)(?: y=(\w+) sums=(\w+) err=(\S+) host32=(\S+) sums_err=(\S+) guard=(\d+))?$", re.M)


def clean_env(extra):
    env = {k: v for k, v in os.environ.items() if k != "BNHIP_EXPDW_FULLW"}
    env.update(extra)
    return env


@pytest.fixture(scope="module")
def check(built_lib, tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("expdw_fullw") / "expdw_fullw_check")
    libdir = os.path.dirname(built_lib)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "birdnet-go_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "ubench", "expdw_fullw_check.cpp"), "-L", libdir, "-lbnhip", "-Wl,-rpath," + libdir],
                   check=True, capture_output=True, timeout=600)
    return exe


def test_eligible_cases_take_the_full_width_form_and_neighbours_do_not(check):
    r = subprocess.run([check, "--list"], capture_output=True, text=True, timeout=120, env=clean_env({}))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    cases = CASE.findall(r.stdout)
    assert len(cases) >= 500 and f"SUMMARY cases={len(cases)} " in r.stdout
    wrong = [c[0] for c in cases if c[1] != c[2]]
    assert not wrong, wrong[:20]
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    # what the list has to contain: every size on every shape in the orientation that fits, the channel widths, both pipes, sums or none
    for k, s, idx in ((3, 1, 2), (5, 1, 6), (5, 2, 12)):
        for h, w in ((6, 32), (5, 32), (3, 32), (6, 31), (6, 33), (6, 64)):
            for hh, ww, shape in ((h, w, idx), (w, h, idx + 22)):
                for cin in (40, 48, 112):
                    for cm in (36, 96):
                        for bx in ("", "_bx"):
                            for sums in ("sums", "nosums"):
                                assert f"k{k}s{s}_{hh}x{ww}/c{cin}x{cm}{bx}/shape{shape}/{sums}" in names
    # the switch restores the footprint mapping everywhere
    r0 = subprocess.run([check, "--list"], capture_output=True, text=True, timeout=120, env=clean_env({"BNHIP_EXPDW_FULLW": "0"}))
    assert r0.returncode == 0 and not [c for c in CASE.findall(r0.stdout) if c[2] != "0"]


@pytest.fixture(scope="module")
def runs(gpu, check):
    """The processes, one after the other, each under its own time limit; nothing more is started after a non-zero exit."""
    outs = []
    for sw in SWITCHES:
        r = subprocess.run(["timeout", "-k", "10", "300", check], capture_output=True, text=True, env=clean_env(sw))
        assert r.returncode == 0, f"{sw}: exit {r.returncode}\n" + "\n".join(r.stdout.splitlines()[-20:]) + r.stderr[-2000:]
        cases = {c[0]: c for c in CASE.findall(r.stdout)}
        assert cases and f"SUMMARY cases={len(cases)} guard_failures=0" in r.stdout, r.stdout[-2000:]
        outs.append(cases)
    return outs


@pytest.mark.gpu
def test_outputs_and_sums_are_bit_identical_without_the_form(runs):
    base, no_fullw = runs
    assert set(base) == set(no_fullw)
    assert any(c[2] == "1" for c in base.values()) and not any(c[2] == "1" for c in no_fullw.values())
    diff = [n for n in base if (base[n][3], base[n][4]) != (no_fullw[n][3], no_fullw[n][4])]
    assert not diff, f"{len(diff)} cases differ under BNHIP_EXPDW_FULLW=0: {diff[:10]}"


@pytest.mark.gpu
def test_every_case_meets_the_fp64_gate(runs):
    worst = 0.0
    for cases in runs:
        for name, c in cases.items():
            err, host32, sums_err = float(c[5]), float(c[6]), float(c[7])
            gate = 4.0 * host32 + 2.0 ** -22
            worst = max(worst, err / gate)
            assert err <= gate, (name, err, host32, gate)
            # the sums as in the lab: per pixel summed, the gate on y plus one rounding at the scale of y
            assert sums_err <= gate + 2.0 ** -24, (name, sums_err, gate)
    print(f"worst error / gate over {sum(len(c) for c in runs)} cases: {worst:.3f}")
