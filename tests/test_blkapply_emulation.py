"""The per-record code of the header-block apply, run on the CPU (no GPU needed).

tests/emu/blkapply_emu.cpp includes the REAL loona_amd/csrc/hpk_blkapply.h as it is (check_record, stage_record,
apply_record, finish_block) behind tests/emu/shim.h, over a table that is a plain array ring, and walks each decoder
as the kernel does. It runs every corpus of blocks_apply_cases.corpora() (the interop stories, the corruptions, the
random and the scan's placed blocks, every truncation of the RFC 7541 App. C blocks on its primed table, the apply's
own placed cases) with a ring of the kernel's size and with a small one that the stories' insertions wrap many times
and that defers more. The answers are blocks_apply_cases.ref_apply's, which tests/test_blocks_apply_cases.py pins to
hpack_ref.Decoder: per block the headers resolved to bytes, the error and its detail; per decoder the blocks applied
and the final table, entry by entry.
The program is also built with -fsanitize=address,undefined and run stand-alone on the same case files."""

import os
import shutil
import struct
import subprocess

import pytest

import blocks_apply_cases as ac
import blocks_scan_cases as bc
import san_util

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
NO_LIMIT = 0xFFFFFFFF


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("blkapply_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(REPO, "loona_amd", "csrc"), "-I",
                           os.path.join(HERE, "emu"), os.path.join(HERE, "emu", "blkapply_emu.cpp"), "-o", str(d / "blkapply_emu")])
    return str(d / "blkapply_emu"), d


def u32(*xs):
    return struct.pack("<%dI" % len(xs), *xs)


def write_cases(path, decoders, ring):
    with open(path, "wb") as f:
        for n, v in ac.static_table():
            f.write(u32(len(n), len(v)) + n + v)
        f.write(u32(len(decoders)))
        for tab, blocks in decoders:
            f.write(u32(tab.max_size, NO_LIMIT if tab.max_allowed is None else tab.max_allowed,
                        ring if tab.cap is None else tab.cap, len(tab.entries)))
            for n, v in tab.entries:
                f.write(u32(len(n), len(v)) + n + v)
            f.write(u32(len(blocks)))
            strs = []
            for w in blocks:
                fields, strings = bc.ref_scan(w)
                f.write(u32(len(fields)))
                for x in fields:
                    f.write(u32(x.index, len(strs) + x.str, x.kind | x.nstr << 8 | x.err << 16 | x.err_stage << 24, x.at))
                strs += ac.decode_strings(w, strings)
            f.write(u32(len(strs)))
            for st, data in strs:
                f.write(u32(st, len(data)) + data)


def pairs(tokens):
    return [tuple(bytes.fromhex(x) for x in t.split(":")) for t in tokens]


_cases = {}


def cases(d, ring):
    """per ring size, made once: the case file both builds of the program read, its decoders, ref_apply's answer and
    the tables after it"""
    if ring not in _cases:
        corp = ac.corpora(ring, 64)
        decoders = [dec for name in sorted(corp) for dec in corp[name]]
        assert len(decoders) > 3900
        path = d / f"cases{ring}.bin"
        write_cases(path, decoders, ring)
        tabs = ac.fresh(decoders)
        _cases[ring] = (str(path), decoders, ac.ref_apply(tabs, ring), tabs)
    return _cases[ring]


def check(p, ring, decoders, want, tabs):
    assert p.returncode == 0 and f"done: {len(decoders)} decoders" in p.stdout, p.stdout[-2000:] + p.stderr
    assert "#" not in p.stdout and "!" not in p.stdout and "\nV" not in p.stdout
    lines = iter(p.stdout.splitlines())
    deferred = errors = 0
    for k, ((results, applied), (tab, blocks)) in enumerate(zip(want, tabs)):
        for b, (headers, error, detail) in enumerate(results):
            x = next(lines).split()
            assert x[0] == "B", (k, b, x[:4])
            assert (int(x[1]), int(x[2]), int(x[3])) == (len(headers), error, detail), (k, b, blocks[b].hex(), x[:4])
            assert pairs(x[4:]) == headers, (k, b, blocks[b].hex())
            deferred += error == ac.E_DEFERRED
            errors += error not in (0, ac.E_DEFERRED)
        x = next(lines).split()
        assert x[0] == "T" and [int(v) for v in x[1:5]] == [applied, len(tab.entries), tab.size, tab.max_size], (k, x[:5])
        assert pairs(x[5:]) == tab.entries, k
    assert errors > 500
    assert deferred >= (8 if ring == 2048 else 10)


@pytest.mark.parametrize("ring", [2048, 128])
def test_step_matches_ref_apply(emu, ring):
    exe, d = emu
    path, *rest = cases(d, ring)
    check(subprocess.run([exe, path, str(ring)], capture_output=True, text=True, timeout=600), ring, *rest)


@pytest.fixture(scope="module")
def emu_san(emu):
    return san_util.build_emu(emu[1], "blkapply_emu_san", san_util.ASAN + ["-Wall"], source="blkapply_emu", oracle=False)


@pytest.mark.parametrize("ring", [2048, 128])
def test_step_under_host_sanitizers(emu, emu_san, ring):
    """The same program with ASan and UBSan, stand-alone, on the same case files and with the same checks."""
    path, *rest = cases(emu[1], ring)
    p = subprocess.run([emu_san, path, str(ring)], capture_output=True, text=True, timeout=600)
    check(p, ring, *rest)
    san_util.assert_no_reports(p)
