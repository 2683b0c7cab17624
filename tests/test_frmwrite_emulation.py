"""The per-thread code of the frame write, run on the CPU (no GPU needed).

tests/emu/frmwrite_emu.cpp includes the REAL loona_amd/csrc/hpk_frmwrite.h as it is (fw_elem, fw_chunk, fw_piece,
fw_header_octet) behind tests/emu/shim.h and drives it tile by tile as the kernel does, the staged arrays read through
a checking accessor, the source ending at a page without access and the destination inside canaries.
  * sweep: M = 1..40, L = 0..3M + 2, every destination alignment 0..15 and source alignment 0..15, the block between
    two neighbours, against a plain frame-by-frame writer in the program, which `plain` mode holds to the model here:
    on the placed cases (the hand-written octets) and on every (M, L) of the sweep;
  * file: batches written here (the placed cases, interop blocks at mixed frame sizes, runs of empty and of void
    blocks longer than the LDS window, a block over three tiles, capacity cuts), compared here with
    frames_write_cases.ref_write_frames, which tests/test_frames_write_cases.py pins to hand-written octets;
  * elems: the length scan's element on synthetic offsets that reach the 64-bit rule.
The program is also built with -fsanitize=address,undefined and run stand-alone on the same inputs."""

import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest

import frames_write_cases as wc
import san_util

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
TILE, LDS = 4096, 1024  # hpk_frmwrite.h: kFwTile, kFwLds (tests/test_gpu_frames_write.py reads them from the library)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("frmwrite_emu")
    with open(os.path.join(REPO, "loona_amd", "csrc", "hpk_frmwrite.h")) as f:
        text = f.read()
    assert f"kFwTile = kFwThreads * 16u, kFwLds = {LDS}" in text and "kFwThreads = 256" in text
    return san_util.build_emu(d, "frmwrite_emu", oracle=False), d


@pytest.fixture(scope="module")
def emu_san(emu):
    exe = san_util.build_emu(emu[1], "frmwrite_emu_san", san_util.ASAN, source="frmwrite_emu", oracle=False)
    assert san_util.has_symbol(exe, "__asan_init")
    return exe


def batches():
    """[(name, items | explicit arrays, src_mis, dst_mis, capacity or None, grid)]"""
    rng = random.Random(5)
    word = lambda: rng.randrange(1, 2**31) | (wc.ES_BIT if rng.random() < 0.3 else 0)  # noqa: E731
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))  # noqa: E731
    out = []
    placed = [(c.block, c.stream_word, c.max_frame) for c in wc.placed()]
    for sm, dm in ((0, 0), (1, 15), (5, 1), (15, 5)):
        out.append(("placed", placed, sm, dm, None, 1 + dm % 3))
    inter = [(b, word(), rng.choice([1, 6, 7, 8, 16, 100, 1024, 16384])) for b in wc.interop_blocks(300)]
    out.append(("interop", inter, 3, 9, None, 7))
    # strides 10, 15, 16, 17 around the 16-byte chunk
    out.append(("strides", [(rb(n), word(), m) for m in (1, 6, 7, 8) for n in range(0, 4 * (m + 9))], 2, 11, None, 2))
    # a header straddling a tile boundary: the second block's header starts 4 octets before it
    first = TILE - 4 - 9 - 6  # its wire length with one frame: + 9
    out.append(("header over a tile edge", [(rb(first), word(), 16384), (rb(40), word(), 16), (rb(3), word(), 5)], 0, 6, None, 2))
    out.append(("one block over three tiles", [(rb(5), word(), 5), (rb(2 * TILE + 100), word(), 1000), (rb(7), word(), 3)], 7, 3, None, 3))
    out.append(("empty blocks in a row", [(rb(9), word(), 4)] + [(b"", word(), 1 + k % 50) for k in range(TILE // 9 + 1)] + [(rb(9), word(), 4)],
                4, 13, None, 2))
    voids = [(rb(20), word(), 7)] + [(b"", word(), 0 if k % 2 else 0x1000000) for k in range(LDS + 5)] + [(rb(20), word(), 7)]
    out.append(("void blocks longer than the window", voids, 1, 2, None, 1))
    x = wc.expected_batch(placed)
    for cap in (x.total - 1, int(x.wire_off[5]) + 4, 17, 0):
        out.append((f"capacity {cap}", placed, 6, 10, cap, 2))
    out.append(("no blocks", [], 0, 0, None, 1))
    return out


def write_file(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for _, items, sm, dm, cap, grid in cases:
            x = wc.expected_batch(items, base=3 if items else 0)
            n = len(items)
            f.write(struct.pack("<6I", n, sm, dm, 0xFFFFFFFF if cap is None else cap, grid, x.blob.size))
            f.write(x.block_off.tobytes() + x.stream_id.tobytes() + x.max_frame.tobytes() + x.blob.tobytes())


def check_file(p, cases):
    san_util.assert_clean(p, f"ok: 0 mismatches in {len(cases)} cases")
    lines = p.stdout.splitlines()
    for k, (name, items, _, _, cap, _) in enumerate(cases):
        x = wc.expected_batch(items, base=3 if items else 0)
        o, s, xx = lines[3 * k : 3 * k + 3]
        assert o[0] == "O" and s[0] == "S" and xx[0] == "X"
        assert [int(t) for t in o.split()[1:]] == x.wire_off.tolist(), name
        assert [int(t) for t in s.split()[1:]] == x.status.tolist(), name
        got = bytes.fromhex(xx[2:])
        want = x.wire.tobytes()
        assert got == (want if cap is None else want[:cap]), name


@pytest.fixture(scope="module")
def case_file(emu):
    cases = batches()
    path = emu[1] / "batches.bin"
    write_file(path, cases)
    return str(path), cases


def elem_records():
    """(a, e, m, cap) records, the model's element for each, and the running verdict"""
    big = 2**32 // 10
    recs = [(0, big + 1, 1, wc.HPK_MAX_OFFSET),  # one block whose wire length passes 2^32
            (0, big - 8, 1, wc.HPK_MAX_OFFSET)]
    recs += [(0, 0, 1, 0), (5, 4, 1, 10), (0, 11, 1, 10), (0, 5, 0, 10), (0, 5, 0x1000000, 10), (0, 5, 0xFFFFFF, 10), (3, 3, 7, 3)]
    recs += [(0, 0x40000000, 0xFFFFFF, 0x40000000)] * 5  # a sum that passes HPK_MAX_OFFSET in its fourth term
    return recs


def model_elem(a, e, m, cap):
    return wc.wire_len(e - a, m) if a <= e <= cap and 1 <= m <= wc.MAX_FRAME_TOP else 0


def check_elems(p, recs):
    san_util.assert_clean(p, f"ok: 0 mismatches in {len(recs)} cases")
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("E ")]
    assert len(lines) == len(recs)
    total = 0
    for (a, e, m, cap), (_, w, s, v) in zip(recs, lines):
        total += model_elem(a, e, m, cap)
        assert (int(w), int(s), int(v)) == (model_elem(a, e, m, cap), total, int(total > wc.HPK_MAX_OFFSET)), (a, e, m, cap)
    return lines


def run_elems(exe, d, name):
    recs = elem_records()
    path = d / name
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(recs)) + b"".join(struct.pack("<4I", *r) for r in recs))
    lines = check_elems(subprocess.run([exe, "elems", str(path)], capture_output=True, text=True, timeout=60), recs)
    assert int(lines[0][1]) > 2**32 and int(lines[0][3]) == 1  # the 64-bit rule is reached by one block alone
    verdicts = [int(x[3]) for x in lines[-5:]]
    assert verdicts[0] == 1  # (the running sum includes the first record)


def test_sweep(emu):
    p = subprocess.run([emu[0], "sweep"], capture_output=True, text=True, timeout=300)
    san_util.assert_clean(p, "ok: 0 mismatches in 660480 cases")


def test_sweep_oracle_is_the_model(emu):
    """the sweep compares with the program's plain writer: that writer gives the placed cases' hand-written octets and
    the model's octets for every (M, L) the sweep visits"""
    rng = random.Random(8)
    placed = [(c.block, c.stream_word, c.max_frame) for c in wc.placed()]
    grid = [(bytes(rng.randrange(256) for _ in range(n)), rng.randrange(2**32), m) for m in range(1, 41) for n in range(3 * m + 3)]
    cases = [("placed", placed, 0, 0, None, 1), ("every M and L of the sweep", grid, 0, 0, None, 1)]
    path = emu[1] / "plain.bin"
    write_file(path, cases)
    p = subprocess.run([emu[0], "plain", str(path)], capture_output=True, text=True, timeout=120)
    san_util.assert_clean(p, "ok: 0 mismatches in 2 cases")
    got = [bytes.fromhex(ln[2:]) for ln in p.stdout.splitlines() if ln.startswith("P ")]
    assert got[0] == b"".join(c.wire for c in wc.placed())
    assert got[1] == b"".join(wc.ref_write_frames(*it) for it in grid) and len(grid) == 2580


def test_batches_match_the_model(emu, case_file):
    check_file(subprocess.run([emu[0], "file", case_file[0]], capture_output=True, text=True, timeout=300), case_file[1])


def test_length_element_reaches_the_64_bit_rule(emu):
    run_elems(emu[0], emu[1], "elems.bin")


def test_sum_alone_passes_max_offset(emu):
    """four blocks of 2^30 octets: no element passes 32 bits, their sum does"""
    recs = [(0, 0x40000000, 0xFFFFFF, 0x40000000)] * 4
    path = emu[1] / "elems_sum.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(recs)) + b"".join(struct.pack("<4I", *r) for r in recs))
    lines = check_elems(subprocess.run([emu[0], "elems", str(path)], capture_output=True, text=True, timeout=60), recs)
    assert [int(x[3]) for x in lines] == [0, 0, 0, 1] and all(int(x[1]) < 2**32 for x in lines)


def test_under_host_sanitizers(emu, emu_san, case_file):
    """The same program with ASan and UBSan, stand-alone, on the same inputs and with the same checks."""
    p = subprocess.run([emu_san, "sweep"], capture_output=True, text=True, timeout=900)
    san_util.assert_clean(p, "ok: 0 mismatches in 660480 cases")
    check_file(subprocess.run([emu_san, "file", case_file[0]], capture_output=True, text=True, timeout=600), case_file[1])
    run_elems(emu_san, emu[1], "elems_san.bin")


def test_batches_cover_their_edges():
    """the batches above reach what they are named for"""
    by_name = {c[0]: c for c in batches()}
    x = wc.expected_batch(by_name["header over a tile edge"][1], base=3)
    dm = by_name["header over a tile edge"][3]
    assert int(x.wire_off[1]) + dm == TILE - 4  # the second block's header straddles coordinates TILE - 4 .. TILE + 5
    x = wc.expected_batch(by_name["one block over three tiles"][1], base=3)
    assert (int(x.wire_off[1]) + 3) // TILE + 2 <= (int(x.wire_off[2]) + 3 - 1) // TILE
    assert np.count_nonzero(wc.expected_batch(by_name["void blocks longer than the window"][1]).status) > LDS
