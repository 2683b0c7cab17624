"""The lane walk on the 13-bit two-symbol table (kTab 4, decode v39) run on the CPU (no GPU needed).

tests/emu/walk13_emu.cpp includes the REAL hpk_walk.h (tests/emu/shim.h stands in for the HIP builtins), as
tests/test_tail_emulation.py does for the 12-bit tables, and runs the 13-bit instantiations of lit12_body,
lit12_tail and the checked step:
  a. tails alone: every bit pattern of 0..18 bits, >= 1M random patterns of 19..30 bits, all ones, all zeros
     and every code of >= 13 bits (EOS too) at every tail offset that shorter codes can reach, followed by ones:
     lit12_tail with its checked fallback gives the image, the output position and the status of the checked
     tail loop from the same state, and writes nothing but the literal's exact-bound region and the dummy slot;
  b. valid tails (codes of <= 13 bits, then 0..7 ones) never take the fallback;
  c. whole literals against the oracle, through the wave kernel's lane protocol and through the checked step
     alone: code bits sweeping 24..48 (the body-min boundary at 29..32), literals made only of the 13-bit pairs
     (6+7, 7+6, 5+8, 8+5) and of the six 13-bit codes (symbols 0, $, @, [, ], ~), and the tail emulation's mix.
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
    """One run (seed 1, 90k random patterns per length 19..30: 1.08M), shared by the tests below."""
    if not shutil.which("g++") or not shutil.which("gcc"):
        pytest.skip("no host C/C++ compiler")
    d = tmp_path_factory.mktemp("walk13_emu")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-D_GNU_SOURCE", "-c", os.path.join(REPO, "oracle", "hpk_oracle.c"),
                           "-o", str(d / "oracle.o")])
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(REPO, "loona_amd", "csrc"), "-I", os.path.join(HERE, "emu"),
                           "-c", os.path.join(HERE, "emu", "walk13_emu.cpp"), "-o", str(d / "walk13_emu.o")])
    subprocess.check_call(["g++", "-o", str(d / "walk13_emu"), str(d / "walk13_emu.o"), str(d / "oracle.o"), "-lpthread"])
    return subprocess.run([str(d / "walk13_emu"), "1", "90000"], capture_output=True, text=True, timeout=300)


def test_tails_match_the_checked_loop(run1):
    assert run1.returncode == 0, run1.stdout + run1.stderr
    m = re.search(r"tails alone: (\d+) cases \((\d+) patterns of 0\.\.18 bits, (\d+) random, (\d+) long-code\), (\d+) slow, "
                  r"(\d+) mismatches", run1.stdout)
    assert m, run1.stdout
    cases, exh, rand, longc, slow, bad = map(int, m.groups())
    assert exh == 2**19 - 1  # every pattern of 0..18 bits
    assert rand >= 1_000_000
    assert longc > 0 and slow > 0  # (a code of >= 14 bits in a tail takes the fallback)
    assert bad == 0


def test_valid_tails_never_slow(run1):
    m = re.search(r"valid tails: (\d+) cases, (\d+) slow", run1.stdout)
    assert m, run1.stdout
    assert int(m.group(1)) > 100000 and int(m.group(2)) == 0, run1.stdout


def test_whole_literals_match_the_oracle(run1):
    m = re.search(r"whole literals: (\d+) literals \((\d+) swept, (\d+) of 13-bit pairs and codes\), (\d+) slow tails, "
                  r"(\d+) mismatches", run1.stdout)
    assert m, run1.stdout
    assert int(m.group(2)) >= 25 * 400 and int(m.group(3)) >= 3000 and int(m.group(5)) == 0, run1.stdout
    assert int(m.group(4)) > 0, "the mix never took the checked fallback"
    assert "ok: 0 mismatches, 0 valid tails slow" in run1.stdout


def test_walk13_emulation_under_host_sanitizers(tmp_path_factory):
    """The same program with ASan and UBSan, stand-alone (another seed, 20k random patterns per length)."""
    if not san_util.have_compilers():
        pytest.skip("no host C/C++ compiler")
    exe = san_util.build_emu(tmp_path_factory.mktemp("walk13_emu_san"), "walk13_emu_san", san_util.ASAN, source="walk13_emu")
    p = subprocess.run([exe, "2", "20000"], capture_output=True, text=True, timeout=300)
    san_util.assert_clean(p, "ok: 0 mismatches, 0 valid tails slow")
    m = re.search(r"tails alone: (\d+) cases \((\d+) patterns of 0\.\.18 bits, (\d+) random, (\d+) long-code\), (\d+) slow, "
                  r"(\d+) mismatches", p.stdout)
    assert m and int(m.group(2)) == 2**19 - 1 and int(m.group(3)) >= 12 * 20000 and int(m.group(6)) == 0, p.stdout
    assert int(m.group(4)) > 0 and int(m.group(5)) > 0, p.stdout
    m = re.search(r"valid tails: (\d+) cases, (\d+) slow", p.stdout)
    assert m and int(m.group(1)) > 100000 and int(m.group(2)) == 0, p.stdout
    m = re.search(r"whole literals: (\d+) literals \((\d+) swept, (\d+) of 13-bit pairs and codes\), (\d+) slow tails, "
                  r"(\d+) mismatches", p.stdout)
    assert m and int(m.group(2)) >= 25 * 400 and int(m.group(3)) >= 3000 and int(m.group(5)) == 0, p.stdout
    assert int(m.group(4)) > 0, "the mix never took the checked fallback"
