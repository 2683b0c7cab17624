"""The wave fills' trimmed tail entry (hpk_wave.h: the saved tail word and the carried status) run on the CPU (no GPU needed).

tests/emu/tailword_emu.cpp includes the REAL hpk_walk.h (tests/emu/shim.h stands in for the HIP builtins), as
tests/test_walk13_emulation.py does, and checks under table kind 4:
  a. tails alone: every bit pattern of 0..16 bits, >= 1M random patterns of 17..30 bits, all ones and all zeros:
     the tail made from the word saved where the lane still held its dwords (tail12_word, tail12_begin_saved)
     equals tail12_begin after lit12_load at the same state, and the status carried out of tail12_end (for a slow
     lane: after its reload and its checked steps) equals residual_status at the stop, or the body's status where
     the body set one;
  b. whole literals through the lane protocol as the kernel runs it now (the first literal's dwords are gone when
     its tail starts; only its slow lanes reload them), exact-bound regions back to back, against the oracle.
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
def run1(tmp_path_factory):
    """One run (seed 1, 80k random patterns per length 17..30: 1.12M), shared by the tests below."""
    if not shutil.which("g++") or not shutil.which("gcc"):
        pytest.skip("no host C/C++ compiler")
    d = tmp_path_factory.mktemp("tailword_emu")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-D_GNU_SOURCE", "-c", os.path.join(REPO, "oracle", "hpk_oracle.c"),
                           "-o", str(d / "oracle.o")])
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(REPO, "loona_amd", "csrc"), "-I", os.path.join(HERE, "emu"),
                           "-c", os.path.join(HERE, "emu", "tailword_emu.cpp"), "-o", str(d / "tailword_emu.o")])
    subprocess.check_call(["g++", "-o", str(d / "tailword_emu"), str(d / "tailword_emu.o"), str(d / "oracle.o"), "-lpthread"])
    return subprocess.run([str(d / "tailword_emu"), "1", "80000"], capture_output=True, text=True, timeout=300)


def test_saved_word_and_carried_status_match(run1):
    assert run1.returncode == 0, run1.stdout + run1.stderr
    m = re.search(r"tails alone: (\d+) cases \((\d+) patterns of 0\.\.16 bits, (\d+) random\), (\d+) slow, (\d+) mismatches",
                  run1.stdout)
    assert m, run1.stdout
    cases, exh, rand, slow, bad = map(int, m.groups())
    assert exh == 2**17 - 1  # every pattern of 0..16 bits
    assert rand >= 1_000_000
    assert slow > 0  # (the slow lanes' reload and their status at the stop were exercised)
    assert bad == 0


def test_whole_literals_match_the_oracle(run1):
    m = re.search(r"whole literals: (\d+) literals, (\d+) slow first tails, (\d+) body statuses, (\d+) mismatches", run1.stdout)
    assert m, run1.stdout
    n, slow, body, bad = map(int, m.groups())
    assert n >= 14000 and bad == 0, run1.stdout
    assert slow > 0 and body > 0, "the mix never took the slow path or never ended in a body"
    assert "ok: 0 mismatches" in run1.stdout


def test_tailword_emulation_under_host_sanitizers(tmp_path_factory):
    """The same program with ASan and UBSan, stand-alone (another seed, 20k random patterns per length)."""
    if not san_util.have_compilers():
        pytest.skip("no host C/C++ compiler")
    exe = san_util.build_emu(tmp_path_factory.mktemp("tailword_emu_san"), "tailword_emu_san", san_util.ASAN, source="tailword_emu")
    p = subprocess.run([exe, "2", "20000"], capture_output=True, text=True, timeout=300)
    san_util.assert_clean(p)
    m = re.search(r"tails alone: (\d+) cases \((\d+) patterns of 0\.\.16 bits, (\d+) random\), (\d+) slow, (\d+) mismatches",
                  p.stdout)
    assert m and int(m.group(2)) == 2**17 - 1 and int(m.group(3)) >= 14 * 20000 and int(m.group(4)) > 0 and int(m.group(5)) == 0, p.stdout
    m = re.search(r"whole literals: (\d+) literals, (\d+) slow first tails, (\d+) body statuses, (\d+) mismatches", p.stdout)
    assert m and int(m.group(1)) >= 14000 and int(m.group(4)) == 0, p.stdout
    assert int(m.group(2)) > 0 and int(m.group(3)) > 0, "the mix never took the slow path or never ended in a body"
