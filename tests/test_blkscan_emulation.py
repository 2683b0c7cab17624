"""The per-lane walk of the header-block scan, run on the CPU (no GPU needed).

tests/emu/blkscan_emu.cpp includes the REAL loona_amd/csrc/hpk_blkscan.h as it is (walk_block) behind
tests/emu/shim.h and runs the count pass and the emit pass on every placed case of blocks_scan_cases, every proper
prefix of the RFC 7541 App. C blocks, the seeded corruptions, the random blocks and a few thousand interop blocks.
The answers are blocks_scan_cases.ref_scan's, which tests/test_blocks_scan_cases.py pins to hpack_ref.Decoder. The
program also checks that count and emit agree, and that no octet outside the block is read: through a checking
accessor, and with the blob at the end of a buffer whose next page has no access, at all 4 dword alignments, with
and without poison bytes after the block.
The program is also built with -fsanitize=address,undefined and run stand-alone on the same case file."""

import os
import shutil
import struct
import subprocess

import pytest

import blocks_scan_cases as bc
import san_util

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("blkscan_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(REPO, "loona_amd", "csrc"), "-I",
                           os.path.join(HERE, "emu"), os.path.join(HERE, "emu", "blkscan_emu.cpp"), "-o", str(d / "blkscan_emu")])
    return str(d / "blkscan_emu"), d


def parse(line):
    x = [int(t) for t in line.split()]
    nf, ns = x[0], x[1]
    assert len(x) == 2 + 7 * nf + 2 * ns
    fields = [bc.Field(*x[2 + 7 * i : 9 + 7 * i]) for i in range(nf)]
    strings = [tuple(x[2 + 7 * nf + 2 * i : 4 + 7 * nf + 2 * i]) for i in range(ns)]
    return fields, strings


@pytest.fixture(scope="module")
def cases(emu):
    """the case file both builds of the program read, its blocks, the placed cases among them (the first ones) and
    ref_scan's answer per block"""
    placed = bc.placed()
    blocks = [b for _, b, _ in placed] + bc.rfc_prefixes() + [w for s in bc.corrupted_stories() for w in s]
    blocks += bc.random_blocks() + bc.interop_blocks()[::5]
    assert len(blocks) > 7000
    path = emu[1] / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(blocks)))
        for w in blocks:
            f.write(struct.pack("<I", len(w)) + w)
    return str(path), blocks, placed, [bc.ref_scan(w) for w in blocks]


def check(p, blocks, placed, wants):
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln and ln[0].isdigit()]
    assert len(lines) == len(blocks) and f"ok: 0 failures in {len(blocks)} cases" in p.stdout
    stages, errs = set(), set()
    for i, (w, ln) in enumerate(zip(blocks, lines)):
        got = parse(ln)
        want = wants[i]
        assert got == (want[0], want[1]), f"block {i} ({w[:16].hex()}..., {len(w)} bytes): {got} for {want}"
        if i < len(placed):
            bc.check_expect(placed[i][0], w, got[0], got[1], placed[i][2])
        if got[0] and got[0][-1].err:
            stages.add(got[0][-1].err_stage)
            errs.add(got[0][-1].err)
    assert stages == {bc.ST_INDEX, bc.ST_NAME, bc.ST_VALUE}
    assert errs == {bc.E_INT_TOO_MANY, bc.E_INT_SHORT, bc.E_STR_SHORT}


def test_walk_matches_ref_scan(emu, cases):
    check(subprocess.run([emu[0], cases[0]], capture_output=True, text=True, timeout=300), *cases[1:])


def test_walk_under_host_sanitizers(emu, cases):
    """The same program with ASan and UBSan, stand-alone, on the same case file and with the same checks."""
    exe = san_util.build_emu(emu[1], "blkscan_emu_san", san_util.ASAN, source="blkscan_emu", oracle=False)
    p = subprocess.run([exe, cases[0]], capture_output=True, text=True, timeout=300)
    check(p, *cases[1:])
    san_util.assert_no_reports(p)
