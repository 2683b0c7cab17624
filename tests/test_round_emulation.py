"""The lane loop's round of nested body steps (lit12_round, decode v41) run on the CPU (no GPU needed).

tests/emu/round_emu.cpp includes the REAL hpk_walk.h (tests/emu/shim.h stands in for the HIP builtins), as
tests/test_walk13_emulation.py does for the 13-bit walk, and replays every case twice from the same state: step
by step with lit12_body (its leading-ones block inline, the walk of decode v27-v40), and round by round with
lit12_round for each way of handling a long code (inline, parked and out of the round, parked and in it). After
every round X, o, st, Eb, the dword pair, `body` and the whole image must be the step walk's after some 1..4 of
its steps; the finished literals are compared with the oracle; nothing but the exact-bound region is written.
  a. every remaining-bit count at a round's start from 0 to 31 + 4 * 26 + 13: the body ends after 0..4 steps;
  b. every code longer than 13 bits, and EOS, as the first and as the second lookup of each of the four steps,
     fitting and cut by the literal's end (PaddingTooLarge, EOSInString);
  c. two long codes in one round;  d. a step that ends the literal exactly;  e. a mix of text and random bytes.
The program is also built with -fsanitize=address,undefined and run stand-alone."""

import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def _build(d, name, flags):
    subprocess.check_call(["gcc", "-O1", "-std=c11", "-D_GNU_SOURCE", *flags, "-c", os.path.join(REPO, "oracle", "hpk_oracle.c"),
                           "-o", str(d / (name + "_oracle.o"))])
    subprocess.check_call(["g++", "-std=c++17", "-O2" if not flags else "-O1", *flags, "-I", os.path.join(REPO, "loona_amd", "csrc"),
                           "-I", os.path.join(HERE, "emu"), "-c", os.path.join(HERE, "emu", "round_emu.cpp"),
                           "-o", str(d / (name + ".o"))])
    subprocess.check_call(["g++", *flags, "-o", str(d / name), str(d / (name + ".o")), str(d / (name + "_oracle.o")), "-lpthread"])
    return str(d / name)


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    if not shutil.which("g++") or not shutil.which("gcc"):
        pytest.skip("no host C/C++ compiler")
    return tmp_path_factory.mktemp("round_emu")


@pytest.fixture(scope="module")
def run1(workdir):
    """One run (seed 1, every symbol), shared by the tests below."""
    exe = _build(workdir, "round_emu", [])
    return subprocess.run([exe, "1", "8"], capture_output=True, text=True, timeout=300)


def test_rounds_match_step_walk_and_oracle(run1):
    assert run1.returncode == 0, run1.stdout + run1.stderr
    assert "ok: 0 mismatches" in run1.stdout
    m = re.search(r"total: (\d+) cases, (\d+) rounds, (\d+) literals against the oracle", run1.stdout)
    assert m and int(m.group(1)) > 200000 and int(m.group(2)) > 200000 and int(m.group(3)) > 100000, run1.stdout


def test_body_ends_after_every_step_count(run1):
    m = re.search(r"sweep: (\d+) cases, first round of (\d+) (\d+) (\d+) (\d+) (\d+) steps", run1.stdout)
    assert m, run1.stdout
    assert int(m.group(1)) == (31 + 4 * 26 + 13 + 1) * 8 * 32  # every bit count, 8 literals each, every X % 32
    assert all(int(g) > 1000 for g in m.groups()[1:]), run1.stdout


def test_long_codes_at_every_lookup_of_the_round(run1):
    m = re.search(r"long codes: (\d+) cases, in the body at ((?:\d+ ?){8}), (\d+) PaddingTooLarge, (\d+) EOSInString", run1.stdout)
    assert m, run1.stdout
    assert all(int(x) > 1000 for x in m.group(2).split()), "a placement (step x first/second lookup) was not reached"
    assert int(m.group(3)) > 1000 and int(m.group(4)) > 100
    m = re.search(r"two long codes: (\d+) cases, (\d+) rounds with two", run1.stdout)
    assert m and int(m.group(2)) > 1000, run1.stdout
    m = re.search(r"exact end: (\d+) cases, (\d+) steps ended a literal exactly", run1.stdout)
    assert m and int(m.group(2)) > 1000, run1.stdout
    m = re.search(r"parked lanes by step: (\d+) (\d+) (\d+) (\d+)", run1.stdout)
    assert m and all(int(g) > 1000 for g in m.groups()), run1.stdout


def test_round_emulation_under_host_sanitizers(workdir):
    """The same program with ASan and UBSan, stand-alone (another seed, every fourth symbol)."""
    exe = _build(workdir, "round_emu_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    p = subprocess.run([exe, "2", "1", "4"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ok: 0 mismatches" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
