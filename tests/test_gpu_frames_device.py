"""hpk_h2_read_frames with the framing on the device (HuffmanCodec.set_frame_scan("device")): tests/test_h2.py's
replay, its single-call form and its error sequences through h2.read_frames, with the same connections' twins on the
default path. Blocks, errors, consumed, hpk_h2conn_error and the decoders' table sizes must be equal between the two
runs, call by call; the replay itself checks the blocks against the fixtures' header lists."""

import ctypes
import random

import pytest

import frames_cases as fc
from h2_cases import BLOCK, C41, CHECK_ORDER, CONNECTION_ERRORS, CONTINUATION, END_HEADERS, HEADERS, interop_connections

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def codecs():
    """(the codec on HPK_FRAME_SCAN_DEVICE, its twin on the default)"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU)")
    from loona_amd import HuffmanCodec

    dev = HuffmanCodec(0, stream=torch.cuda.current_stream())
    host = HuffmanCodec(0, stream=torch.cuda.current_stream())
    dev.set_frame_scan("device")
    yield dev, host
    for c in (dev, host):
        c.set_frame_scan("host")
        c.set_block_scan("host")
        c.set_block_apply("host")
        c.close()


def table_size(conn):
    from loona_amd import _lib

    L = _lib.lib()
    a, b, c = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.hpk_hdec_table_size(L.hpk_h2conn_decoder(conn._h), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
    return a.value, b.value, c.value


def state(conns):
    return [(c.error, table_size(c)) for c in conns]


def both(codecs, conns_dev, conns_host, chunks):
    """one call on each path -> the device path's result, after comparing everything with the default path's"""
    from loona_amd import h2

    dev, host = codecs
    a = h2.read_frames(conns_dev, chunks, dev)
    b = h2.read_frames(conns_host, chunks, host)
    assert a.errors == b.errors and a.consumed == b.consumed
    assert len(a.blocks) == len(b.blocks)
    for i, (x, y) in enumerate(zip(a.blocks, b.blocks)):
        assert x[:3] == y[:3], i
        assert x[3] == y[3] or (getattr(x[3], "kind", 0) == getattr(y[3], "kind", 1) and x[3].detail == y[3].detail), (i, x[3], y[3])
    assert state(conns_dev) == state(conns_host)
    return a


def test_set_frame_scan_arguments(codecs):
    from loona_amd import _lib

    dev, host = codecs
    with pytest.raises(ValueError):
        host.set_frame_scan("gpu")
    assert _lib.lib().hpk_ctx_set_frame_scan(host._h, 2) == _lib.HPK_E_INVAL
    assert _lib.lib().hpk_ctx_set_frame_scan(None, 1) == _lib.HPK_E_INVAL


@pytest.mark.parametrize("settings", ["plain", "block scan on the device", "block apply on the device"])
def test_replay_in_four_random_cuts(codecs, settings):
    """tests/test_h2.py's replay, both paths side by side: the same cuts, the incomplete frames sent again"""
    from loona_amd import h2

    dev, host = codecs
    for c in codecs:  # (the twin takes the same block path: only the framing differs)
        c.set_block_scan("device" if settings == "block scan on the device" else "host")
        c.set_block_apply("device" if settings == "block apply on the device" else "host")
    try:
        seed, calls = 11, 4
        rng = random.Random(seed + 1)
        wires, wants = interop_connections(seed)
        if settings != "plain":
            wires, wants = wires[::3], wants[::3]
        cd, ch = [h2.Connection() for _ in wires], [h2.Connection() for _ in wires]
        cuts = [sorted(rng.sample(range(len(w) + 1), calls - 1)) + [len(w)] for w in wires]
        pos = [0] * len(wires)
        got = [[] for _ in wires]
        for k in range(calls):
            chunks = [wires[c][pos[c] : cuts[c][k]] for c in range(len(wires))]
            res = both(codecs, cd, ch, chunks)
            assert res.errors == [None] * len(wires)
            for c in range(len(wires)):
                pos[c] += res.consumed[c]
            for conn, sid, es, val in res.blocks:
                got[conn].append((sid, es, val))
        assert pos == [len(w) for w in wires]
        assert got == wants
    finally:
        for c in codecs:
            c.set_block_scan("host")
            c.set_block_apply("host")


def test_single_call_many_connections(codecs):
    from loona_amd import h2

    wires, wants = interop_connections(7)
    cd, ch = [h2.Connection() for _ in wires], [h2.Connection() for _ in wires]
    res = both(codecs, cd, ch, wires)
    assert res.errors == [None] * len(wires) and res.consumed == [len(w) for w in wires]
    got = [[] for _ in wires]
    for conn, sid, es, val in res.blocks:
        got[conn].append((sid, es, val))
    assert got == wants
    # no connections, and connections with no bytes
    assert both(codecs, [], [], []).blocks == []
    assert both(codecs, cd[:3], ch[:3], [b"", b"", b""]).consumed == [0, 0, 0]


def test_error_sequences_in_one_call_and_afterwards(codecs):
    """every CHECK_ORDER and CONNECTION_ERRORS sequence on a connection of its own, good connections between them,
    all in one call; then a second call: the errors are sticky and the good connections go on"""
    from loona_amd import h2

    seqs = [(h2.frame(HEADERS, 0, 1, BLOCK[:5]) + second, err) for second, err in CHECK_ORDER]
    seqs += [(b"".join(frames), err) for frames, err, _ in CONNECTION_ERRORS]
    good = h2.frame(HEADERS, END_HEADERS, 1, BLOCK)
    chunks, want = [], []
    for data, err in seqs:
        chunks += [data, good]
        want += [err, None]
    cd, ch = [h2.Connection() for _ in chunks], [h2.Connection() for _ in chunks]
    res = both(codecs, cd, ch, chunks)
    assert res.errors == want and [c.error for c in cd] == want
    assert [b for b in res.blocks if b[0] % 2 == 1] == [(k, 1, False, C41) for k in range(1, len(chunks), 2)]
    assert [b for b in res.blocks if b[0] % 2 == 0] == []
    again = h2.frame(HEADERS, END_HEADERS, 3, bytes.fromhex("828684be"))  # entry 62: C.4.1's authority
    res = both(codecs, cd, ch, [again] * len(chunks))
    assert res.errors == want
    assert res.consumed == [0 if e else len(again) for e in want]
    assert res.blocks == [(k, 3, False, C41) for k in range(1, len(chunks), 2)]


def test_placed_cases_with_their_carry_over_two_calls(codecs):
    """the placed cases that enter pending: the first call leaves the block open with the carry held, the second is
    the case's bytes; both paths agree call by call"""
    from loona_amd import h2

    cases = [c for c in fc.placed() if c.state.pending and not c.state.error]
    assert len(cases) >= 6
    cd = [h2.Connection(c.state.max_frame_size) for c in cases]
    ch = [h2.Connection(c.state.max_frame_size) for c in cases]
    first = [h2.frame(HEADERS, 0x1 if c.state.pend_stream >> 31 else 0, c.state.pend_stream & 0x7FFFFFFF, c.carry) for c in cases]
    res = both(codecs, cd, ch, first)
    assert res.blocks == [] and res.errors == [None] * len(cases)
    res = both(codecs, cd, ch, [c.data for c in cases])
    assert res.consumed == [c.expect.consumed for c in cases]
    assert res.errors == [h2.ERRORS[c.expect.error] if c.expect.error else None for c in cases]
    assert [(b[0], b[1], b[2]) for b in res.blocks] == [(k, s, bool(e)) for k, c in enumerate(cases) for s, e, _ in c.expect.blocks]
    # a third call completes what is still open
    tail = [h2.frame(CONTINUATION, END_HEADERS, c.expect.pending[0], b"") if c.expect.pending and not c.expect.error else b"" for c in cases]
    both(codecs, cd, ch, tail)


def test_compression_error_and_skipped_blocks(codecs):
    from loona_amd import h2

    bad = h2.frame(HEADERS, END_HEADERS, 1, b"\x40")
    good = h2.frame(HEADERS, END_HEADERS, 3, BLOCK)
    cd, ch = [h2.Connection(), h2.Connection()], [h2.Connection(), h2.Connection()]
    r = both(codecs, cd, ch, [bad + good, good])
    assert r.errors == ["HpackDecodingError", None]
    assert [(x[0], x[1], x[3] is None) for x in r.blocks] == [(0, 1, False), (0, 3, True), (1, 3, False)]
    r = both(codecs, cd, ch, [good, good])
    assert r.errors == ["HpackDecodingError", None] and r.consumed[0] == 0


def test_a_forced_failure_leaves_the_connections_untouched(codecs):
    """hpk_test_fail_batches fails the device frame scan as a device error would: the call fails, and the connections
    (a block pending with bytes held, a table with an entry) are where they were: the same call again gives what the
    twins give"""
    from loona_amd import _lib, h2

    dev, host = codecs
    cd, ch = [h2.Connection(), h2.Connection()], [h2.Connection(), h2.Connection()]
    first = [h2.frame(HEADERS, END_HEADERS, 1, BLOCK) + h2.frame(HEADERS, 0, 3, BLOCK[:4]), h2.frame(HEADERS, 0, 1, BLOCK[:9])]
    both(codecs, cd, ch, first)
    before = state(cd)
    second = [h2.frame(CONTINUATION, END_HEADERS, 3, BLOCK[4:]), h2.frame(CONTINUATION, END_HEADERS, 1, BLOCK[9:]) + h2.frame(0x0, 0x8, 1, b"")]
    _lib.lib().hpk_test_fail_batches(1)
    try:
        with pytest.raises(RuntimeError, match="injected"):
            h2.read_frames(cd, second, dev)
    finally:
        _lib.lib().hpk_test_fail_batches(0)
    assert state(cd) == before
    r = both(codecs, cd, ch, second)
    assert r.errors == [None, "PaddedFrameEmpty"] and [b[1:] for b in r.blocks] == [(3, False, C41), (1, False, C41)]


def test_a_connection_listed_twice_is_refused(codecs):
    from loona_amd import h2

    dev, _ = codecs
    c = h2.Connection()
    good = h2.frame(HEADERS, END_HEADERS, 1, BLOCK)
    with pytest.raises(RuntimeError):
        h2.read_frames([c, c], [good, good], dev)
    assert c.error is None and h2.read_frames([c], [good], dev).blocks == [(0, 1, False, C41)]
