"""The per-lane walk of the frame scan, run on the CPU (no GPU needed).

tests/emu/frmscan_emu.cpp includes the REAL loona_amd/csrc/hpk_frmscan.h as it is (walk_frames) behind
tests/emu/shim.h and runs the count pass and the emit pass on every placed case of frames_cases, on the interop
connections cut at random points over several calls (the held bytes re-fed as the carry) and on the seeded
corruptions of frame headers. The answers are frames_cases.ref_scan_frames', which tests/test_frames_cases.py pins
to the hand-written expectations and to h2_cases._frames. The program also checks that count and emit agree, and
that no octet outside the connection's range is read: through a checking accessor, and with the blob at the end of
a buffer whose next page has no access, at all 4 dword alignments, with and without poison bytes after the
connection, the carry window poisoned.
The program is also built with -fsanitize=address,undefined and run stand-alone on the same case file."""

import os
import random
import shutil
import struct
import subprocess

import pytest

import frames_cases as fc
import h2_cases as hc
import san_util

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("frmscan_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(REPO, "loona_amd", "csrc"), "-I",
                           os.path.join(HERE, "emu"), os.path.join(HERE, "emu", "frmscan_emu.cpp"), "-o", str(d / "frmscan_emu")])
    return str(d / "frmscan_emu"), d


def cut_calls(seed, every, calls=4):
    """(state, data, carry) of every call of the interop connections sent in random cuts"""
    rng = random.Random(seed)
    wires, _ = hc.interop_connections(seed)
    out = []
    for w in wires[::every]:
        cuts = fc.cut_points(rng, len(w), calls)
        state, carry, pos = fc.State(), b"", 0
        for k in range(calls):
            data = w[pos : cuts[k]]
            out.append((state, data, carry))
            scan = fc.ref_scan_frames(state, data, carry)
            _, carry = fc.scan_blocks_bytes(scan, data, carry)
            state, pos = scan.state, pos + scan.consumed
        assert pos == len(w)
    return out


@pytest.fixture(scope="module")
def cases(emu):
    """the case file both builds of the program read, its (state, data, carry) items, the placed cases among them
    (the first ones) and ref_scan_frames' answer per item"""
    placed = fc.placed()
    items = [(c.state, c.data, c.carry) for c in placed]
    items += cut_calls(0, 2) + cut_calls(1, 3, calls=7)
    items += [(fc.State(), w, b"") for w in fc.corrupted_wires()]
    items += [(fc.State(16384, 0, 1, 3), w, b"abc") for w in fc.corrupted_wires(seed=6, n=100)]
    assert len(items) > 1000
    path = emu[1] / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(items)))
        for st, data, carry in items:
            f.write(struct.pack("<IiIIII", st.max_frame_size, st.error, st.pending, st.pend_stream, len(carry), len(data)) + data)
    return str(path), items, placed, [fc.ref_scan_frames(*it) for it in items]


def parse(line):
    x = [int(t) for t in line.split()]
    nb, nf, no, consumed, err, pending, pend_stream = x[:7]
    assert len(x) == 7 + 3 * nb + 2 * nf
    blocks = [tuple(x[7 + 3 * i : 10 + 3 * i]) for i in range(nb)]
    frags = [tuple(x[7 + 3 * nb + 2 * i : 9 + 3 * nb + 2 * i]) for i in range(nf)]
    return blocks, frags[: nf - no], frags[nf - no :], consumed, err, pending, pend_stream


def check(p, items, placed, wants):
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln and ln[0].isdigit()]
    assert len(lines) == len(items) and f"ok: 0 failures in {len(items)} cases" in p.stdout
    errs, carried = set(), 0
    for i, ((st, data, carry), ln, want) in enumerate(zip(items, lines, wants)):
        blocks, closed, opened, consumed, err, pending, pend_stream = parse(ln)
        got = fc.Scan(blocks, closed, opened, fc.State(st.max_frame_size, err, pending, pend_stream), consumed)
        assert got == want, f"case {i} ({len(data)} bytes, {st}): {got} for {want}"
        if i < len(placed):
            fc.check_expect(placed[i], got)
        errs.add(err)
        carried += bool(st.pending and blocks)
    assert errs == set(range(9)) and carried > 50


def test_walk_matches_ref_scan_frames(emu, cases):
    check(subprocess.run([emu[0], cases[0]], capture_output=True, text=True, timeout=300), *cases[1:])


def test_walk_under_host_sanitizers(emu, cases):
    """The same program with ASan and UBSan, stand-alone, on the same case file and with the same checks."""
    exe = san_util.build_emu(emu[1], "frmscan_emu_san", san_util.ASAN, source="frmscan_emu", oracle=False)
    p = subprocess.run([exe, cases[0]], capture_output=True, text=True, timeout=300)
    check(p, *cases[1:])
    san_util.assert_no_reports(p)
