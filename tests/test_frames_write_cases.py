"""The frame write's model and its host form (no GPU needed).

frames_write_cases.ref_write_frames is pinned to the hand-written octets of placed() and to the frame scan's model
(frames_cases.ref_scan_frames, itself pinned to h2_cases._frames): what the one writes, the other reads back as the
same block on the same stream, in as many fragments as frames. Then hpk_write_frames_cpu is pinned to the model,
with its HPK_E_INVAL and capacity rules."""

import ctypes
import random

import numpy as np
import pytest

import frames_cases as fc
import frames_write_cases as wc
from loona_amd import _lib, h2

E_INVAL, E_NOSPACE = -1, -2


@pytest.mark.parametrize("case", wc.placed(), ids=lambda c: c.name)
def test_model_gives_the_placed_octets(case):
    assert wc.ref_write_frames(case.block, case.stream_word, case.max_frame) == case.wire
    assert wc.frame_count(len(case.block), case.max_frame) == case.frames
    assert wc.wire_len(len(case.block), case.max_frame) == len(case.wire)


def scan_back(block, word, m):
    wire = wc.ref_write_frames(block, word, m)
    assert len(wire) == wc.wire_len(len(block), m)
    scan = fc.ref_scan_frames(fc.State(m), wire, b"")
    nfr = wc.frame_count(len(block), m)
    assert scan.blocks == [(word, 0, nfr)], (scan.blocks, word, nfr)
    assert len(scan.closed) == nfr and not scan.open
    assert scan.consumed == len(wire) and scan.state == fc.State(m, 0, 0, scan.state.pend_stream)
    got, held = fc.scan_blocks_bytes(scan, wire, b"")
    assert got == [(word & 0x7FFFFFFF, word >> 31, bytes(block))] and held == b""
    # the limit is tight: every frame but the last is exactly m octets long
    assert [n for _, n in scan.closed[:-1]] == [m] * (nfr - 1)


def test_scan_reads_back_what_the_model_writes_placed():
    for c in wc.placed():
        scan_back(c.block, c.stream_word, c.max_frame)


def test_scan_reads_back_what_the_model_writes_interop():
    rng = random.Random(3)
    blocks = wc.interop_blocks()
    assert len(blocks) > 1000
    for i, b in enumerate(blocks[::7]):
        for m in (1, 7, 16, len(b) or 1, max(len(b) - 1, 1), len(b) + 1, 16384):
            scan_back(b, (2 * i + 1) | (wc.ES_BIT if rng.random() < 0.5 else 0), m)


def run_cpu(x, out_cap=None):
    return h2.write_frames_cpu(x.blob, x.block_off, x.stream_id, x.max_frame, out_cap)


def test_cpu_matches_the_model_placed():
    x = wc.expected_batch([(c.block, c.stream_word, c.max_frame) for c in wc.placed()], base=3)
    out, woff, st, rc = run_cpu(x)
    assert rc == 0 and np.array_equal(woff, x.wire_off) and not st.any()
    assert out.tobytes() == x.wire.tobytes() == b"".join(c.wire for c in wc.placed())


def test_cpu_matches_the_model_interop():
    rng = random.Random(11)
    blocks = wc.interop_blocks(600)
    items = [(b, rng.randrange(1, 2**31) | (wc.ES_BIT if rng.random() < 0.3 else 0), rng.choice([1, 6, 7, 8, 16, 100, 16384, 0xFFFFFF]))
             for b in blocks]
    x = wc.expected_batch(items)
    out, woff, st, rc = run_cpu(x)
    assert rc == 0 and np.array_equal(woff, x.wire_off) and not st.any()
    assert np.array_equal(out, x.wire)


def test_cpu_capacity_rules():
    x = wc.expected_batch([(c.block, c.stream_word, c.max_frame) for c in wc.placed()])
    inside_header = int(x.wire_off[5]) + 4  # four octets into a HEADERS frame's header
    for cap in (x.total - 1, inside_header, 9, 1, 0):
        out, woff, st, rc = run_cpu(x, cap)
        assert rc == E_NOSPACE, cap
        assert np.array_equal(woff, x.wire_off) and not st.any()
        assert np.array_equal(out[:cap], x.wire[:cap])
    # a larger buffer: nothing at or past the total is written
    out, woff, st, rc = run_cpu(x, x.total + 32)
    assert rc == 0 and np.array_equal(out[: x.total], x.wire) and (out[x.total :] == 0xA5).all()


def test_cpu_no_blocks():
    out, woff, st, rc = h2.write_frames_cpu(np.zeros(0, np.uint8), np.array([7], np.uint32)[:1] * 0, [], [], 4)
    assert rc == 0 and woff.tolist() == [0] and (out == 0xA5).all()


@pytest.mark.parametrize("what", ["decreasing", "past cap", "M = 0", "M = 0x1000000"])
def test_cpu_inval_writes_nothing(what):
    items = [(b"abc", 1, 5), (b"defgh", 3, 2), (b"", 5, 5)]
    x = wc.expected_batch(items)
    off, mf = x.block_off.copy(), x.max_frame.copy()
    if what == "decreasing":
        off[1] = 9
        off[2] = 8
        off[3] = 8
    elif what == "past cap":
        off[3] = 9
    elif what == "M = 0":
        mf[1] = 0
    else:
        mf[2] = 0x1000000
    blob = np.concatenate([x.blob, np.zeros(8, np.uint8)])[: 8 if what != "decreasing" else 16]
    L = _lib.lib()
    out = np.full(64, 0xA5, np.uint8)
    woff = np.full(4, 0xDEAD, np.uint32)
    st = np.full(3, 0x77, np.uint8)
    rc = L.hpk_write_frames_cpu(blob.ctypes.data, blob.size, off.ctypes.data, 3, x.stream_id.ctypes.data, mf.ctypes.data,
                                out.ctypes.data, out.size, woff.ctypes.data, st.ctypes.data)
    assert rc == E_INVAL
    assert (out == 0xA5).all() and (woff == 0xDEAD).all() and (st == 0x77).all()


def test_cpu_cap_above_max_offset_and_total_past_it():
    L = _lib.lib()
    one = np.zeros(16, np.uint8)
    off = np.array([0, 4], np.uint32)
    sid = np.array([1], np.uint32)
    mf = np.array([1], np.uint32)
    out = np.full(16, 0xA5, np.uint8)
    woff = np.full(2, 0xDEAD, np.uint32)
    st = np.full(1, 0x77, np.uint8)
    args = (off.ctypes.data, 1, sid.ctypes.data, mf.ctypes.data, out.ctypes.data, out.size, woff.ctypes.data, st.ctypes.data)
    assert L.hpk_write_frames_cpu(one.ctypes.data, ctypes.c_size_t(wc.HPK_MAX_OFFSET + 1), *args) == E_INVAL
    assert (woff == 0xDEAD).all() and (out == 0xA5).all()
    # one block of 2^32 / 10 octets at M = 1 passes HPK_MAX_OFFSET on the wire: void, and no octet of it is read
    big = 2**32 // 10 + 1
    assert wc.wire_len(big, 1) > wc.HPK_MAX_OFFSET >= wc.wire_len(big - 8, 1)
    off[1] = big
    assert L.hpk_write_frames_cpu(one.ctypes.data, ctypes.c_size_t(big), *args) == E_INVAL
    assert woff.tolist() == [0, 0] and st.tolist() == [wc.HPK_BAD_OFFSETS] and (out == 0xA5).all()
