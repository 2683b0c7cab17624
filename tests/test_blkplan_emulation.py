"""The per-header code of the header-block plan, run on the CPU (no GPU needed).

tests/emu/blkplan_emu.cpp includes the REAL loona_amd/csrc/hpk_blkplan.h as it is (hash, test_entry, combine, build,
the checks) and hpk_blkapply.h's insert behind tests/emu/shim.h, over a table that is a plain array ring, and walks
each encoder as the kernel does, the 64 lanes of a search step run in a loop. It runs every corpus of
blocks_plan_cases.corpora() (the interop stories' header lists, the random lists, the placed cases with their hash
collisions) with a ring of the kernel's size and with one of 128 records that the stories wrap many times and that
defers more. The answers are blocks_plan_cases.ref_plan's, which tests/test_blocks_plan_cases.py pins to
hpack_ref.Encoder: per header the kind, the index, the prefix octets and the three items resolved to bytes; per
encoder the blocks planned and the final table, entry by entry.
The program is also built with -fsanitize=address,undefined and run stand-alone on the case files the runs above wrote."""

import os
import shutil
import struct
import subprocess

import pytest

import blocks_apply_cases as ac
import blocks_plan_cases as pc
import san_util

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("blkplan_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(REPO, "loona_amd", "csrc"), "-I",
                           os.path.join(HERE, "emu"), os.path.join(HERE, "emu", "blkplan_emu.cpp"), "-o", str(d / "blkplan_emu")])
    return str(d / "blkplan_emu"), d


def u32(*xs):
    return struct.pack("<%dI" % len(xs), *xs)


def write_cases(path, encoders, ring):
    with open(path, "wb") as f:
        for n, v in ac.static_table():
            f.write(u32(len(n), len(v)) + n + v)
        f.write(u32(len(encoders)))
        for tab, blocks, huffman in encoders:
            f.write(u32(tab.max_size, max(ring, len(tab.entries)) if tab.cap is None else tab.cap, int(huffman), len(tab.entries)))
            for n, v in tab.entries:
                f.write(u32(len(n), len(v)) + n + v)
            f.write(u32(len(blocks)))
            for blk in blocks:
                f.write(u32(len(blk)) + b"".join(u32(len(n), len(v)) + n + v for n, v in blk))


def parse_header(token):
    kind, index, prefix, *items = token.split(",")
    return int(kind), int(index), bytes.fromhex(prefix), [(int(p), bytes.fromhex(s)) for p, s in (it.split(":") for it in items)]


def pairs(tokens):
    return [tuple(bytes.fromhex(x) for x in t.split(":")) for t in tokens]


_wants = {}


def run_emu(emu, encoders, ring, tag, exe=None):
    """the emulation over `encoders`, checked against ref_plan on copies of the tables -> (the tables as the emulation
    printed them, the deferred blocks, the planned headers). exe: another build of the program, run on the case file
    and against the answer that the call without it made under the same tag."""
    d = emu[1]
    path = d / f"cases{tag}.bin"
    if exe is None:
        write_cases(path, encoders, ring)
        tabs = pc.fresh(encoders)
        _wants[tag] = (pc.ref_plan(tabs, ring), tabs)
    want, tabs = _wants[tag]
    p = subprocess.run([exe or emu[0], str(path), str(ring)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and f"done: {len(encoders)} encoders" in p.stdout, p.stdout[-2000:] + p.stderr
    assert "#" not in p.stdout and "!" not in p.stdout and "\nV" not in p.stdout
    if exe is not None:
        san_util.assert_no_reports(p)
    lines = iter(p.stdout.splitlines())
    deferred = headers = 0
    after = []
    for k, ((results, planned), (tab, blocks, _)) in enumerate(zip(want, tabs)):
        for b, res in enumerate(results):
            x = next(lines).split()
            if res is None:
                assert x == ["D"], (k, b, x[:3])
                deferred += 1
                continue
            assert x[0] == "B" and [parse_header(t) for t in x[1:]] == res, (k, b, blocks[b][:4])
            headers += len(res)
        x = next(lines).split()
        assert x[0] == "T" and [int(v) for v in x[1:5]] == [planned, len(tab.entries), tab.size, tab.max_size], (k, x[:5])
        assert pairs(x[5:]) == tab.entries, k
        after.append(ac.Table(pairs(x[5:]), int(x[4]), None, tab.cap))
    return after, deferred, headers


@pytest.mark.parametrize("calls", [2, 3])
def test_calls_carry_the_tables(emu, calls):
    """the table one call prints goes into the next as its carried-in entries, against the model carried likewise"""
    ring = 128
    stories, model = pc.carried(ring)
    tabs = [t.copy() for t in model]
    for c in range(calls):
        part = [blocks[len(blocks) * c // calls : len(blocks) * (c + 1) // calls] for blocks, _ in stories]
        tabs, _, _ = run_emu(emu, [(t, p, h) for t, p, (_, h) in zip(tabs, part, stories)], ring, f"carry{calls}_{c}")
        pc.ref_plan([(t, p, h) for t, p, (_, h) in zip(model, part, stories)], ring)
        assert [(t.entries, t.size, t.max_size) for t in tabs] == [(t.entries, t.size, t.max_size) for t in model]
    assert sum(len(t.entries) for t in tabs) > 0


@pytest.mark.parametrize("ring", [2048, 128])
def test_step_matches_ref_plan(emu, ring):
    corp = pc.corpora(ring, 64, 64)
    encoders = [enc for name in sorted(corp) for enc in corp[name]]
    assert len(encoders) > 500
    _, deferred, headers = run_emu(emu, encoders, ring, ring)
    assert headers > 190000
    # the deferral cases' four blocks; with the small ring also the twelve search cases' and the two index cases' tables
    assert deferred >= (4 if ring == 2048 else 18)


@pytest.fixture(scope="module")
def emu_san(emu):
    return san_util.build_emu(emu[1], "blkplan_emu_san", san_util.ASAN + ["-Wall"], source="blkplan_emu", oracle=False)


@pytest.mark.parametrize("ring", [2048, 128])
def test_step_under_host_sanitizers(emu, emu_san, ring):
    """The same program with ASan and UBSan, stand-alone, on the same corpora and with the same checks."""
    exe = emu_san
    corp = pc.corpora(ring, 64, 64)
    encoders = [enc for name in sorted(corp) for enc in corp[name]]
    if ring not in _wants:  # (run alone: the unsanitized run writes the case file and makes the model's answer)
        run_emu(emu, encoders, ring, ring)
    _, deferred, headers = run_emu(emu, encoders, ring, ring, exe=exe)
    assert headers > 190000 and deferred >= (4 if ring == 2048 else 18)
