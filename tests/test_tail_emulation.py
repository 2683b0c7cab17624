"""The wave fills' masked tail (lit12_tail, decode v38) run on the CPU (no GPU needed).

tests/emu/tail_emu.cpp includes the REAL hpk_walk.h (tests/emu/shim.h stands in for the HIP builtins), as
tests/test_walk_emulation.py does for the walk, and checks:
  a. tails alone: every bit pattern of 0..16 bits, >= 1M random patterns of 17..28 bits, all ones, all
     zeros and every 13..28-bit code followed by ones, behind random window bits and at every X % 32:
     lit12_tail with its checked fallback gives the image, the output position and the status of the
     checked tail loop (lit12_step<.., kMore>) from the same state, and writes nothing but the literal's
     exact-bound region and the dummy slot;
  b. valid tails (codes of <= 12 bits, then 0..7 ones: every sequence of code lengths, and random symbol
     sequences) never take the fallback;
  c. whole literals: the wave kernel's lane protocol (body steps, masked tails, checked steps for the slow
     lanes) on the walk emulation's literal mix, exact-bound regions back to back, against the oracle.
The program is also built with -fsanitize=address,undefined and run stand-alone: each fill's window is an allocation of
exactly the dwords the walk may read, one guard dword in front included, and every fill runs with that dword all zeros
and all ones (lit12_load's contract, hpk_walk.h)."""

import os
import re
import shutil
import subprocess

import pytest

import san_util

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def tail_emu(tmp_path_factory):
    if not shutil.which("g++") or not shutil.which("gcc"):
        pytest.skip("no host C/C++ compiler")
    d = tmp_path_factory.mktemp("tail_emu")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-D_GNU_SOURCE", "-c", os.path.join(REPO, "oracle", "hpk_oracle.c"),
                           "-o", str(d / "oracle.o")])
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(REPO, "loona_amd", "csrc"), "-I", os.path.join(HERE, "emu"),
                           "-c", os.path.join(HERE, "emu", "tail_emu.cpp"), "-o", str(d / "tail_emu.o")])
    subprocess.check_call(["g++", "-o", str(d / "tail_emu"), str(d / "tail_emu.o"), str(d / "oracle.o"), "-lpthread"])
    return str(d / "tail_emu")


@pytest.fixture(scope="module")
def run1(tail_emu):
    """One run (seed 1, 100k random patterns per length 17..28: 1.2M), shared by the tests below."""
    p = subprocess.run([tail_emu, "1", "4", "100000"], capture_output=True, text=True, timeout=300)
    return p


def test_masked_tail_matches_checked_loop_and_oracle(run1):
    assert run1.returncode == 0, run1.stdout + run1.stderr
    m = re.search(r"tails alone: (\d+) cases, (\d+) slow, (\d+) mismatches", run1.stdout)
    assert m, run1.stdout
    # exhaustive 0..16 bits at 32 alignments in both table layouts, and >= 1M random longer ones
    assert int(m.group(1)) >= 2 * 32 * (2**17 - 1) + 1_200_000
    assert int(m.group(3)) == 0
    m = re.search(r"whole literals: (\d+) literals, (\d+) slow tails, (\d+) mismatches", run1.stdout)
    assert m and int(m.group(1)) >= 20000 and int(m.group(3)) == 0, run1.stdout
    assert int(m.group(2)) > 0, "the mix never took the checked fallback"
    assert "ok: 0 mismatches" in run1.stdout


def test_valid_tails_never_slow(run1):
    ms = re.findall(r"valid tails tab (\d): (\d+) cases, (\d+) slow", run1.stdout)
    assert len(ms) == 2, run1.stdout
    for tab, cases, slow in ms:
        assert int(cases) > 100000 and int(slow) == 0, run1.stdout


def test_masked_tail_second_seed(tail_emu):
    p = subprocess.run([tail_emu, "2", "2", "20000"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ok: 0 mismatches, 0 valid tails slow" in p.stdout


def test_masked_tail_under_host_sanitizers(tmp_path_factory):
    """The same program with ASan and UBSan, stand-alone (the second seed's workload)."""
    if not san_util.have_compilers():
        pytest.skip("no host C/C++ compiler")
    exe = san_util.build_emu(tmp_path_factory.mktemp("tail_emu_san"), "tail_emu_san", san_util.ASAN, source="tail_emu")
    p = subprocess.run([exe, "2", "2", "20000"], capture_output=True, text=True, timeout=300)
    san_util.assert_clean(p, "ok: 0 mismatches, 0 valid tails slow")
    m = re.search(r"tails alone: (\d+) cases, (\d+) slow, (\d+) mismatches", p.stdout)
    assert m and int(m.group(1)) >= 2 * 32 * (2**17 - 1) + 12 * 20000 and int(m.group(3)) == 0, p.stdout
    m = re.search(r"whole literals: (\d+) literals, (\d+) slow tails, (\d+) mismatches", p.stdout)
    assert m and int(m.group(1)) >= 2 * 6000 and int(m.group(3)) == 0, p.stdout  # (two rounds of 3,000 literals per table)
    assert int(m.group(2)) > 0, "the mix never took the checked fallback"
    ms = re.findall(r"valid tails tab (\d): (\d+) cases, (\d+) slow", p.stdout)
    assert len(ms) == 2 and all(int(cases) > 100000 and int(slow) == 0 for _, cases, slow in ms), p.stdout
