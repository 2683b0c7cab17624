"""What one lane of the small-call mode's persistent kernel does for one literal, run on the CPU (no GPU needed).

tests/emu/persist_emu.cpp includes the REAL hpk_persist_lit.h (tests/emu/shim.h stands in for the HIP language), as
tests/test_tail_emulation.py does for the wave fills' tail, and runs the kernel's staged-or-global test (restated
from hpk_persist.h, where it has to stay) and the function it chooses, one lane at a time, against the oracle:
  a. the store plan, exhaustive: every (out_mis + o0) mod 16 x every decoded count 0..180 on the staged bound path;
  b. input placement: every (in_mis + p0) mod 16 x lengths 1..113 x the literal mix of test_gpu_tail.py, with the
     reference's error vectors of at most 113 bytes;
  c. every case of b twice, with 0xFF and with random bytes around the literal, in the slots and behind the slot;
  d. short regions: a sample of b's literals at every capacity 0 .. bound - 1, against the oracle at that capacity;
  e. the global walker: lengths 114..300 and three of 1-4 KiB at every output residue mod 8 and input residue mod
     16, capacities bound, count, count - 1, count - 2 and 0;
  f. the dispatch: 113 bytes staged at every misalignment in at most 8 chunks, 114 bytes never.
Every case: the oracle's status, length and bytes, and no byte outside the literal's region changed.
Finding of c, modelled in the program and explained in its header: the lane walk reads up to three dwords past its
33-dword input slot (in the kernel the next lane's first dwords); they never decide anything.
The program is also built with -fsanitize=address,undefined and run stand-alone."""

import os
import re
import shutil
import struct
import subprocess

import pytest

import san_util
from hpk_util import load

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SLOT_MAX = 113


@pytest.fixture(scope="module")
def persist_emu(tmp_path_factory):
    if not shutil.which("g++") or not shutil.which("gcc"):
        pytest.skip("no host C/C++ compiler")
    d = tmp_path_factory.mktemp("persist_emu")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-D_GNU_SOURCE", "-c", os.path.join(REPO, "oracle", "hpk_oracle.c"),
                           "-o", str(d / "oracle.o")])
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(REPO, "loona_amd", "csrc"), "-I", os.path.join(HERE, "emu"),
                           "-c", os.path.join(HERE, "emu", "persist_emu.cpp"), "-o", str(d / "persist_emu.o")])
    subprocess.check_call(["g++", "-o", str(d / "persist_emu"), str(d / "persist_emu.o"), str(d / "oracle.o"), "-lpthread"])
    return str(d / "persist_emu")


@pytest.fixture(scope="module")
def vectors(tmp_path_factory):
    """the reference's error vectors of at most 113 bytes (every 8th: 16 placements each), as the program reads them"""
    vecs = [bytes.fromhex(k["in"]) for k in load("kat.json") if k["status"] != 0]
    vecs += [bytes.fromhex(v["in"]) for v in load("error_vectors.json")["vectors"] if v["status"] != 0][::8]
    vecs = [v for v in vecs if 0 < len(v) <= SLOT_MAX]
    assert len(vecs) >= 100
    path = tmp_path_factory.mktemp("persist_vec") / "vectors.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(vecs)))
        for v in vecs:
            f.write(struct.pack("<I", len(v)) + v)
    return str(path), len(vecs)


@pytest.fixture(scope="module")
def run1(persist_emu, vectors):
    return subprocess.run([persist_emu, "1", vectors[0]], capture_output=True, text=True, timeout=600)


def nums(pattern, text):
    m = re.search(pattern, text)
    assert m, text
    return [int(x) for x in m.groups()]


def test_zero_mismatches_and_case_counts(run1, vectors):
    out = run1.stdout
    assert run1.returncode == 0, out + run1.stderr
    nvec = vectors[1]
    cases, bad, *pieces = nums(r"a store plan: (\d+) cases, (\d+) mismatches; pieces taken: head (\d+) lead (\d+) groups (\d+) "
                               r"trail (\d+) tail (\d+)", out)
    assert (cases, bad) == (16 * 181 * 4, 0)
    cases, vec, bad = nums(r"b input placement: (\d+) cases \((\d+) error vectors\), (\d+) mismatches", out)
    assert (cases, vec, bad) == (16 * SLOT_MAX * 8 + 16 * nvec, nvec, 0)
    pairs, bad, past = nums(r"c independence: (\d+) pairs, (\d+) mismatches, (\d+) may read past", out)
    assert (pairs, bad) == (cases, 0)
    lits, cases, bad, behind, at = nums(r"d short regions: (\d+) literals, (\d+) cases, (\d+) mismatches; error behind the "
                                        r"capacity (\d+), at it (\d+)", out)
    # (every 6th of b's 14,464 + nvec literals; lengths 1..113 evenly: a mean bound of 91 capacities each)
    assert lits >= 2000 and cases >= 80 * lits and bad == 0
    assert behind > 0 and at > 0, "no literal whose error comes after the capacity is reached"
    cases, bad, guard = nums(r"e global walker: (\d+) cases, (\d+) mismatches, (\d+) at capacity count - 1 or count - 2", out)
    # (lengths 114..300 x 8 x 16 placements and 3 x 16 long ones, 5 capacities each, fewer where count < 2)
    assert 4 * (187 * 128 + 48) <= cases <= 5 * (187 * 128 + 48) and bad == 0 and guard >= cases // 4
    cases, bad = nums(r"f dispatch: (\d+) cases, (\d+) mismatches", out)
    assert (cases, bad) == ((4096 + 16) * 115, 0)
    assert "ok: 0 mismatches" in out


def test_every_path_and_store_piece_taken(run1):
    out = run1.stdout
    paths = nums(r"paths: empty (\d+) staged_bound (\d+) staged_bytes (\d+) global (\d+)", out)
    assert all(p > 0 for p in paths), out
    pieces = nums(r"pieces taken: head (\d+) lead (\d+) groups (\d+) trail (\d+) tail (\d+)", out)
    assert all(p > 0 for p in pieces), out
    past = nums(r"(\d+) may read past", out)[0]
    assert past > 0, "no literal ends in its eighth chunk's last bytes: the reads behind the slot are not exercised"


def test_second_seed(persist_emu):
    p = subprocess.run([persist_emu, "2", "-"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ok: 0 mismatches" in p.stdout


def test_persist_emulation_under_host_sanitizers(tmp_path_factory):
    """The same program with ASan and UBSan, stand-alone (the second seed, without the error vectors: the program has
    no smaller workload). Its slots are malloc'd at their exact sizes, so a read past one is a report."""
    if not san_util.have_compilers():
        pytest.skip("no host C/C++ compiler")
    exe = san_util.build_emu(tmp_path_factory.mktemp("persist_emu_san"), "persist_emu_san", san_util.ASAN, source="persist_emu")
    p = subprocess.run([exe, "2", "-"], capture_output=True, text=True, timeout=600)
    san_util.assert_clean(p)
    paths = nums(r"paths: empty (\d+) staged_bound (\d+) staged_bytes (\d+) global (\d+)", p.stdout)
    assert all(x > 0 for x in paths), p.stdout
