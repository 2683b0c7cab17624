"""The per-lane decode code of the GPU kernels, run on the CPU (no GPU needed).

tests/emu/emu.cpp includes the REAL per-lane headers of loona_amd/csrc as they are (hpk_walk.h:
lit12_body, lit12_step with its end detection, lit12_load/status, lo_decode; hpk_huge_piece.h: the
huge-literal phase's per-piece functions); tests/emu/shim.h, included first, stands in for the handful
of HIP builtins they use (alignbit, clz). tests/emu/emu.cpp replays the kernels' per-lane protocols — the
wave kernel's body steps then both tails (LUT3 and LUT2), the fill kernel's (LUT2), the huge-literal
phase's passes and fix rounds (under LUT2, LUT3 and the wave kernel's 13-bit table; a fix loop that does not
end within P + 2 rounds fails) — on random literals (text, 5-bit-only text that reaches the decoded
bound, random bytes, EOS runs, bad and too-long padding) in exact-bound regions back to back, against
the oracle (oracle/hpk_oracle.c, the checker). What it cannot cover — LDS, waves, the fills' staging —
is the GPU suite's job (tests/test_gpu.py).
The program is also built with -fsanitize=address,undefined and run stand-alone: each fill's window is then an
allocation of exactly the dwords the walk may read, one guard dword in front included (lit12_load's contract)."""

import os
import shutil
import subprocess

import pytest

import san_util

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    if not shutil.which("g++") or not shutil.which("gcc"):
        pytest.skip("no host C/C++ compiler")
    return tmp_path_factory.mktemp("emu")


@pytest.fixture(scope="module")
def emu(workdir):
    d = workdir
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-D_GNU_SOURCE", "-c", os.path.join(REPO, "oracle", "hpk_oracle.c"),
                           "-o", str(d / "oracle.o")])
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(REPO, "loona_amd", "csrc"), "-I", os.path.join(HERE, "emu"),
                           "-c", os.path.join(HERE, "emu", "emu.cpp"), "-o",
                           str(d / "emu.o")])
    subprocess.check_call(["g++", "-o", str(d / "emu"), str(d / "emu.o"), str(d / "oracle.o"), "-lpthread"])
    return str(d / "emu")


@pytest.mark.parametrize("seed", [1, 2])
def test_lane_walk_emulation_matches_oracle(emu, seed):
    p = subprocess.run([emu, str(seed), "6"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ok: 0 mismatches" in p.stdout


def test_lane_walk_emulation_under_host_sanitizers(workdir):
    """The same program with ASan and UBSan, stand-alone (another seed, two rounds of the lane protocols and eight
    huge literals). The parent of this test's commit aborted here: lit12_load's read of the dword before a window
    that starts with a literal fell in front of the allocation."""
    exe = san_util.build_emu(workdir, "emu_san", san_util.ASAN, source="emu")
    p = subprocess.run([exe, "3", "2"], capture_output=True, text=True, timeout=300)
    san_util.assert_clean(p)
