"""frames_cases.ref_scan_frames, the model the frame scan's tests compare against, pinned before they use it (no GPU
needed): to the hand-written expectations of frames_cases.placed(), and to h2_cases._frames, the framing model that
tests/test_h2.py's sequences and tests/test_host_sanitizers.py are written against, on the placed cases and on the
interop connections cut at random points over several calls with the carry fed back between the calls."""

import random

import pytest

import frames_cases as fc
import h2_cases as hc


@pytest.fixture(scope="module")
def placed():
    return fc.placed()


def ref_conn(state, carry):
    c = hc.RefConn(state.max_frame_size)
    c.error = state.error
    if state.pending:
        c.pending = (state.pend_stream & 0x7FFFFFFF, state.pend_stream >> 31, bytes(carry))
    return c


def same_as_frames(state, data, carry, scan):
    """ref_scan_frames' answer against h2_cases._frames on the same state and bytes -> the bytes held afterwards"""
    conn = ref_conn(state, carry)
    blocks, pos, err = hc._frames(conn, bytes(data))
    got, held = fc.scan_blocks_bytes(scan, data, carry)
    assert got == [(sid, es, bytes(b)) for sid, es, b in blocks]
    assert scan.consumed == pos and scan.state.error == err
    assert bool(scan.state.pending) == (conn.pending is not None)
    if conn.pending is not None:
        assert (scan.state.pend_stream & 0x7FFFFFFF, scan.state.pend_stream >> 31, held) == conn.pending
    else:
        assert held == b"" and not scan.open
    return held


def test_placed_cases_meet_their_expectations(placed):
    for case in placed:
        fc.check_expect(case, fc.ref_scan_frames(case.state, case.data, case.carry))
        # the windows move with the data and with the carry
        fc.check_expect(case, fc.ref_scan_frames(case.state, case.data, case.carry, 1000, 7), 1000, 7)


def test_placed_cases_equal_the_framing_model(placed):
    for case in placed:
        same_as_frames(case.state, case.data, case.carry, fc.ref_scan_frames(case.state, case.data, case.carry))


def test_placed_cases_reach_their_edges(placed):
    """every error code but COMPRESSION_ERROR, both padded types, both ends of each comparison"""
    by = {c.name: c for c in placed}
    assert {c.expect.error for c in placed} == set(range(9))
    assert len(placed) >= 50
    # the comparisons' two sides are both there
    for a, b in (("len == max_frame_size, payload absent", "len == max_frame_size + 1, payload absent"),
                 ("PADDED HEADERS, pad == n - 1", "PADDED HEADERS, pad == n"), ("PADDED DATA, pad == n - 1", "PADDED DATA, pad == n"),
                 ("PRIORITY, 5 octets", "PRIORITY, 4 octets"),
                 ("PADDED and PRIORITY, 5 octets left after the padding", "PADDED and PRIORITY, 4 octets left after the padding")):
        assert by[a].expect.error == 0 and by[b].expect.error != 0
    assert len(by["end: 8 bytes left"].data) - by["end: 8 bytes left"].expect.consumed == 8
    assert len(by["end: 9 bytes left, len > 0"].data) - by["end: 9 bytes left, len > 0"].expect.consumed == 9
    assert by["22 empty fragments"].expect.closed_lens == [0] * (len(by["22 empty fragments"].data) // 9)
    assert any(c.state.pending and not c.carry and c.expect.blocks for c in placed)
    assert any(c.state.pending and c.carry and c.expect.blocks for c in placed)
    assert any(c.state.pending and c.carry and not c.expect.blocks and c.expect.error == 0 for c in placed)
    assert any(c.state.error and c.expect.consumed == 0 for c in placed)
    assert any(c.expect.blocks and c.expect.pending for c in placed)
    assert sum(c.name.startswith("check order") for c in placed) == len(hc.CHECK_ORDER) == 5
    assert sum(c.name.startswith("connection error") for c in placed) == len(hc.CONNECTION_ERRORS)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_interop_connections_in_random_cuts(seed):
    """the interop wires over several calls: an incomplete frame is sent again, the held bytes are the next carry"""
    rng = random.Random(seed)
    wires, wants = hc.interop_connections(seed)
    calls = 5
    nblocks = 0
    for w, want in list(zip(wires, wants))[:: 1 + seed]:
        cuts = fc.cut_points(rng, len(w), calls)
        state, carry, pos, got = fc.State(), b"", 0, []
        twin = hc.RefConn()
        for k in range(calls):
            data = w[pos : cuts[k]]
            scan = fc.ref_scan_frames(state, data, carry)
            held = same_as_frames(state, data, carry, scan)
            tb, tpos, terr = hc._frames(twin, data)  # the model carried through all the calls by itself
            blocks, _ = fc.scan_blocks_bytes(scan, data, carry)
            assert blocks == tb and scan.consumed == tpos and terr == 0
            got += blocks
            state, carry, pos = scan.state, held, pos + scan.consumed
        assert pos == len(w) and not state.pending
        assert [(s, bool(e)) for s, e, _ in got] == [(s, e) for s, e, _ in want]
        nblocks += len(got)
    assert nblocks > 2000


def test_corrupted_headers_equal_the_framing_model():
    errs = set()
    for w in fc.corrupted_wires():
        scan = fc.ref_scan_frames(fc.State(), w, b"")
        same_as_frames(fc.State(), w, b"", scan)
        errs.add(scan.state.error)
    assert len(errs) >= 6


def test_expected_batch_lays_the_cases_out(placed):
    items = [(c.state, c.data, c.carry) for c in placed]
    for base in (0, 3):
        x = fc.expected_batch(items, base)
        assert len(x.blocks) == sum(len(c.expect.blocks) for c in placed) == x.conn_blk_off[-1]
        assert [bytes(b) for b in x.block_bytes] == [b for c in placed for _, _, b in c.expect.blocks]
        assert list(x.conns_out["error"]) == [c.expect.error for c in placed]
        assert list(x.conns_out["consumed"]) == [c.expect.consumed for c in placed]
        # the fragments of block b are frag .. frag + nfrag of the closed list and read the blob
        raw = x.blob.tobytes()
        for b, want in zip(x.blocks, x.block_bytes):
            f, n = int(b["frag"]), int(b["nfrag"])
            assert b"".join(raw[int(o) : int(o) + int(m)] for o, m in zip(x.frag_off[f : f + n], x.frag_len[f : f + n])) == want
        for k, c in enumerate(placed):
            held = b"".join(raw[int(o) : int(o) + int(m)] for o, m in
                            zip(x.open_off[x.conn_open_off[k] : x.conn_open_off[k + 1]], x.open_len[x.conn_open_off[k] : x.conn_open_off[k + 1]]))
            assert held == c.expect.held, c.name
