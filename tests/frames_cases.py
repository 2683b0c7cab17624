"""The frame scan's cases (hpk_scan_frames, hpk_frame_blocks) and a model of its walk.

ref_scan_frames restates the per-connection walk of loona_amd/csrc/hpk_frmscan.h, step 1 of hpk_h2_read_frames: the
deframer's length check and padding removal (crates/loona/src/h2/server.rs:290-390), the HEADERS priority block
(:895-911) and the CONTINUATION gathering (:1299-1303, :1349-1417). It gives what the scan gives: block records,
closed and open fragment windows and the new state. tests/test_frames_cases.py pins it to h2_cases._frames (the model
tests/test_h2.py's sequences are written against) and to the hand-written expectations of placed() before the
emulation and the GPU tests use it.

placed() is written from RFC 9113 (section 4.1 the frame header, 4.2 the size limit, 6.1 / 6.2 padding and the
priority block, 6.10 CONTINUATION) and the cited server.rs lines, never from the model."""

import random
from collections import namedtuple

import numpy as np

import h2_cases as hc
from h2_cases import BLOCK, CONTINUATION, DATA, END_HEADERS, END_STREAM, HEADERS, PADDED, PING, PRIO, frame

FCONN_DTYPE = np.dtype([("max_frame_size", "<u4"), ("error", "<i4"), ("pending", "<u4"), ("pend_stream", "<u4"),
                        ("carry_off", "<u4"), ("carry_len", "<u4"), ("consumed", "<u4"), ("status", "<u4")])
FBLOCK_DTYPE = np.dtype([("conn", "<u4"), ("stream_id", "<u4"), ("frag", "<u4"), ("nfrag", "<u4")])
ES_BIT = 0x80000000

State = namedtuple("State", "max_frame_size error pending pend_stream")  # pend_stream: bit 31 = END_STREAM
State.__new__.__defaults__ = (16384, 0, 0, 0)
# blocks: [(stream_id | END_STREAM << 31, first fragment, fragment count)]; closed / open: [(offset, length)]
Scan = namedtuple("Scan", "blocks closed open state consumed")


def _be31(b):
    return int.from_bytes(b[:4], "big") & 0x7FFFFFFF


def ref_scan_frames(state, data, carry, base=0, carry_at=None):
    """One connection's walk. `data` lies at offset `base` of the blob; a connection that enters pending has the
    window (carry_at, len(carry)) as its fragment 0 (carry_at defaults to the end of the data)."""
    data = bytes(data)
    if carry_at is None:
        carry_at = base + len(data)
    frags, blocks = [], []
    first, pos, err = 0, 0, state.error
    pending, pend_stream = state.pending, state.pend_stream
    if pending:
        frags.append((carry_at, len(carry)))
    while err == 0 and len(data) - pos >= 9:
        length, ftype, flags, sid = int.from_bytes(data[pos : pos + 3], "big"), data[pos + 3], data[pos + 4], _be31(data[pos + 5 :])
        if length > state.max_frame_size:  # server.rs:318-325: not consumed
            err = hc.FRAME_TOO_LARGE
            break
        if len(data) - pos - 9 < length:
            break
        p, n = pos + 9, length
        pos += 9 + length
        if ftype in (DATA, HEADERS) and flags & PADDED:  # server.rs:356-382
            if n == 0:
                err = hc.PADDED_FRAME_EMPTY
                break
            pad = data[p]
            p, n = p + 1, n - 1
            if n < pad:
                err = hc.PADDED_FRAME_TOO_SHORT
                break
            n -= pad
        if pending:  # server.rs:1376-1417
            if sid != pend_stream & 0x7FFFFFFF:
                err = hc.EXPECTED_CONTINUATION_FOR_STREAM
                break
            if ftype != CONTINUATION:
                err = hc.EXPECTED_CONTINUATION_FRAME
                break
            frags.append((base + p, n))
            if flags & END_HEADERS:
                blocks.append((pend_stream, first, len(frags) - first))
                pending, first = 0, len(frags)
            continue
        if ftype == CONTINUATION:  # server.rs:1299-1303
            err = hc.UNEXPECTED_CONTINUATION_FRAME
            break
        if ftype != HEADERS:
            continue
        if flags & PRIO:  # server.rs:895-911
            if n < 5:
                err = hc.PRIORITY_PARSE
                break
            if _be31(data[p:]) == sid:
                err = hc.HEADERS_INVALID_PRIORITY
                break
            p, n = p + 5, n - 5
        sid_es = sid | (ES_BIT if flags & END_STREAM else 0)
        frags.append((base + p, n))
        if flags & END_HEADERS:
            blocks.append((sid_es, first, 1))
            first = len(frags)
        else:
            pending, pend_stream = 1, sid_es
    nclosed = first if pending else len(frags)
    return Scan(blocks, frags[:nclosed], frags[nclosed:], State(state.max_frame_size, err, pending, pend_stream), pos)


def window_bytes(win, data, carry, base=0, carry_at=None):
    """the bytes of one fragment window of ref_scan_frames(state, data, carry, base, carry_at)"""
    if carry_at is None:
        carry_at = base + len(data)
    off, n = win
    if n == 0:
        return b""
    if base <= off and off + n <= base + len(data):  # (the carry window never overlaps the data)
        return bytes(data[off - base : off - base + n])
    assert carry_at <= off and off + n <= carry_at + len(carry), (win, base, len(data), carry_at, len(carry))
    return bytes(carry[off - carry_at : off - carry_at + n])


def scan_blocks_bytes(scan, data, carry, base=0, carry_at=None):
    """[(stream, end_stream, block bytes)] of a Scan, and the bytes its open fragments hold"""
    wb = lambda w: window_bytes(w, data, carry, base, carry_at)  # noqa: E731
    out = [(sid & 0x7FFFFFFF, sid >> 31, b"".join(wb(w) for w in scan.closed[f : f + n])) for sid, f, n in scan.blocks]
    return out, b"".join(wb(w) for w in scan.open)


# ---- the placed cases -------------------------------------------------------------------------------------------
# what a case must give, written by hand: blocks [(stream, end_stream, bytes)], the connection error, the bytes
# consumed, the pending block after the call (stream, end_stream) or None, the bytes held for it, and the lengths of
# the closed and of the open fragments in order
Expect = namedtuple("Expect", "blocks error consumed pending held closed_lens open_lens")
Case = namedtuple("Case", "name state data carry expect")

B = BLOCK  # 17 octets
H1 = frame(HEADERS, END_HEADERS, 1, B)  # 26 octets


def raw_header(length, ftype, flags, sid32):
    """a frame header alone, the stream id's 32 bits as given (the reserved bit included)"""
    return length.to_bytes(3, "big") + bytes([ftype, flags]) + sid32.to_bytes(4, "big")


def placed():
    c = []

    def add(name, data, expect, state=State(), carry=b""):
        c.append(Case(name, state, bytes(data), bytes(carry), expect))

    one = [(1, 0, B)]
    # bytes left at the connection's end (RFC 9113 section 4.1: a frame header is 9 octets)
    add("end: 0 bytes left", H1, Expect(one, 0, 26, None, b"", [17], []))
    nxt = frame(HEADERS, END_HEADERS, 3, B)
    add("end: 8 bytes left", H1 + nxt[:8], Expect(one, 0, 26, None, b"", [17], []))
    add("end: 9 bytes left, len > 0", H1 + nxt[:9], Expect(one, 0, 26, None, b"", [17], []))
    add("end: one byte short of a payload", H1 + nxt[:-1], Expect(one, 0, 26, None, b"", [17], []))
    add("end: fewer than 9 bytes in all", nxt[:5], Expect([], 0, 0, None, b"", [], []))
    add("no bytes", b"", Expect([], 0, 0, None, b"", [], []))
    # the frame length at the limit (section 4.2; server.rs:318-325 checks before the payload is there)
    add("len == max_frame_size, payload absent", raw_header(16384, DATA, 0, 1), Expect([], 0, 0, None, b"", [], []))
    add("len == max_frame_size + 1, payload absent", raw_header(16385, DATA, 0, 1),
        Expect([], hc.FRAME_TOO_LARGE, 0, None, b"", [], []))
    add("len == max_frame_size + 1 after a block", H1 + raw_header(16385, HEADERS, END_HEADERS, 3) + b"xx",
        Expect(one, hc.FRAME_TOO_LARGE, 26, None, b"", [17], []))
    add("len == max_frame_size, payload present", frame(DATA, 0, 1, b"d" * 16384) + H1,
        Expect(one, 0, 9 + 16384 + 26, None, b"", [17], []))
    big = State(16777215)
    add("max_frame_size 16777215: the largest length, payload absent", raw_header(0xFFFFFF, HEADERS, END_HEADERS, 1) + b"abc",
        Expect([], 0, 0, None, b"", [], []), state=big)
    add("max_frame_size 16777215: a 20000-octet frame", frame(DATA, 0, 1, b"d" * 20000) + H1,
        Expect(one, 0, 9 + 20000 + 26, None, b"", [17], []), state=big)
    add("max_frame_size 16384: the same frame", frame(DATA, 0, 1, b"d" * 20000) + H1,
        Expect([], hc.FRAME_TOO_LARGE, 0, None, b"", [], []))
    # padding (sections 6.1, 6.2; server.rs:356-382)
    add("PADDED HEADERS, n == 0", frame(HEADERS, END_HEADERS | PADDED, 1, b""), Expect([], hc.PADDED_FRAME_EMPTY, 9, None, b"", [], []))
    add("PADDED DATA, n == 0", frame(DATA, PADDED, 1, b"") + H1, Expect([], hc.PADDED_FRAME_EMPTY, 9, None, b"", [], []))
    add("PADDED HEADERS, pad == n - 1", frame(HEADERS, END_HEADERS | PADDED, 1, bytes([3]) + b"\0" * 3),
        Expect([(1, 0, b"")], 0, 13, None, b"", [0], []))
    add("PADDED HEADERS, pad == n", frame(HEADERS, END_HEADERS | PADDED, 1, bytes([4]) + b"\0" * 3),
        Expect([], hc.PADDED_FRAME_TOO_SHORT, 13, None, b"", [], []))
    add("PADDED DATA, pad == n - 1", frame(DATA, PADDED, 1, bytes([3]) + b"\0" * 3) + H1, Expect(one, 0, 39, None, b"", [17], []))
    add("PADDED DATA, pad == n", frame(DATA, PADDED, 1, bytes([4]) + b"\0" * 3) + H1,
        Expect([], hc.PADDED_FRAME_TOO_SHORT, 13, None, b"", [], []))
    add("PADDED HEADERS with a block", frame(HEADERS, END_HEADERS | PADDED | END_STREAM, 7, bytes([2]) + B + b"\0\0"),
        Expect([(7, 1, B)], 0, 9 + 20, None, b"", [17], []))
    add("PADDED on CONTINUATION is not padding", frame(HEADERS, 0, 1, B[:5]) + frame(CONTINUATION, END_HEADERS | PADDED, 1, B[5:]),
        Expect(one, 0, 14 + 21, None, b"", [5, 12], []))
    add("PADDED on an empty CONTINUATION is not an error", frame(HEADERS, 0, 1, B) + frame(CONTINUATION, END_HEADERS | PADDED, 1, b""),
        Expect(one, 0, 26 + 9, None, b"", [17, 0], []))
    # the priority block (section 6.2; server.rs:895-911)
    add("PRIORITY, 4 octets", frame(HEADERS, END_HEADERS | PRIO, 1, b"\0\0\0\x03"), Expect([], hc.PRIORITY_PARSE, 13, None, b"", [], []))
    add("PRIORITY, 5 octets", frame(HEADERS, END_HEADERS | PRIO, 1, b"\0\0\0\x03\x10"), Expect([(1, 0, b"")], 0, 14, None, b"", [0], []))
    add("PRIORITY, dependency == stream", frame(HEADERS, END_HEADERS | PRIO, 1, b"\0\0\0\x01\x10" + B),
        Expect([], hc.HEADERS_INVALID_PRIORITY, 9 + 22, None, b"", [], []))
    add("PRIORITY, dependency == stream with the exclusive bit", frame(HEADERS, END_HEADERS | PRIO, 1, b"\x80\0\0\x01\x10" + B),
        Expect([], hc.HEADERS_INVALID_PRIORITY, 9 + 22, None, b"", [], []))
    add("PRIORITY, another dependency with the exclusive bit", frame(HEADERS, END_HEADERS | PRIO, 1, b"\x80\0\0\x03\x10" + B),
        Expect(one, 0, 9 + 22, None, b"", [17], []))
    add("PADDED and PRIORITY, 4 octets left after the padding",
        frame(HEADERS, END_HEADERS | PADDED | PRIO, 1, bytes([2]) + b"\0\0\0\x03" + b"\0\0"), Expect([], hc.PRIORITY_PARSE, 9 + 7, None, b"", [], []))
    add("PADDED and PRIORITY, 5 octets left after the padding",
        frame(HEADERS, END_HEADERS | PADDED | PRIO, 1, bytes([2]) + b"\0\0\0\x03\x10" + b"\0\0"), Expect([(1, 0, b"")], 0, 9 + 8, None, b"", [0], []))
    # the five CHECK_ORDER sequences (server.rs:1391-1397 before :1399-1408): both frames are consumed, the block stays open
    head = frame(HEADERS, 0, 1, B[:5])
    for second, err in hc.CHECK_ORDER:
        add(f"check order: {err} ({second[3]}, stream {second[8]})", head + second,
            Expect([], hc.H2_NAMES[err], len(head) + len(second), (1, 0), B[:5], [], [5]))
    # every entry of CONNECTION_ERRORS: (consumed, pending, held, open lengths) by hand
    by_hand = [
        (14 + 21, (1, 0), B[:5], [5]),  # HEADERS then CONTINUATION of stream 3
        (9, None, b"", []),             # PADDED HEADERS with no payload
        (9 + 18, None, b"", []),        # pad 40 of 17 octets
        (9, None, b"", []),             # PADDED DATA with no payload
        (9 + 22, None, b"", []),        # dependency on itself
        (9 + 2, None, b"", []),         # 2 octets of priority
        (26, None, b"", []),            # CONTINUATION with nothing pending
        (0, None, b"", []),             # 16385 octets: not consumed
    ]
    assert len(by_hand) == len(hc.CONNECTION_ERRORS)
    for (frames, err, _), (consumed, pend, held, olens) in zip(hc.CONNECTION_ERRORS, by_hand):
        add(f"connection error: {err} ({len(frames)} frames, type {frames[0][3]})", b"".join(frames),
            Expect([], hc.H2_NAMES[err], consumed, pend, held, [], olens))
    # pending on entry, and the carry
    pend5 = State(16384, 0, 1, 5 | ES_BIT)
    add("pending, carry of 0 bytes, completed", frame(CONTINUATION, END_HEADERS, 5, B), Expect([(5, 1, B)], 0, 26, None, b"", [0, 17], []),
        state=pend5)
    add("pending, carry of 4 bytes, completed", frame(CONTINUATION, END_HEADERS, 5, B[4:]), Expect([(5, 1, B)], 0, 22, None, b"", [4, 13], []),
        state=pend5, carry=B[:4])
    add("pending, carry of 0 bytes, not completed", frame(CONTINUATION, 0, 5, B[:3]), Expect([], 0, 12, (5, 1), B[:3], [], [0, 3]),
        state=pend5)
    add("pending, carry of 4 bytes, not completed", frame(CONTINUATION, 0, 5, B[4:9]), Expect([], 0, 14, (5, 1), B[:9], [], [4, 5]),
        state=pend5, carry=B[:4])
    add("pending, carry of 4 bytes, no frame arrives", frame(CONTINUATION, 0, 5, B[4:9])[:8], Expect([], 0, 0, (5, 1), B[:4], [], [4]),
        state=pend5, carry=B[:4])
    add("pending, completed, then a block and another left open",
        frame(CONTINUATION, END_HEADERS, 5, B[4:]) + H1 + frame(HEADERS, 0, 9, B[:2]),
        Expect([(5, 1, B), (1, 0, B)], 0, 22 + 26 + 11, (9, 0), B[:2], [4, 13, 17], [2]), state=pend5, carry=B[:4])
    add("pending, another stream's HEADERS", frame(HEADERS, END_HEADERS, 7, B),
        Expect([], hc.EXPECTED_CONTINUATION_FOR_STREAM, 26, (5, 1), B[:4], [], [4]), state=pend5, carry=B[:4])
    # a chain of zero-length CONTINUATION frames: nine bytes per fragment, the fragment bound
    chain = frame(HEADERS, 0, 1, b"") + frame(CONTINUATION, 0, 1, b"") * 20 + frame(CONTINUATION, END_HEADERS, 1, b"")
    add("22 empty fragments", chain, Expect([(1, 0, b"")], 0, 22 * 9, None, b"", [0] * 22, []))
    add("21 empty fragments left open", chain[: 21 * 9], Expect([], 0, 21 * 9, (1, 0), b"", [], [0] * 21))
    # a block left open after completed ones
    add("a block left open after two completed", H1 + frame(HEADERS, END_HEADERS, 3, B) + frame(HEADERS, END_STREAM, 5, B[:7]) +
        frame(CONTINUATION, 0, 5, B[7:9]), Expect([(1, 0, B), (3, 0, B)], 0, 26 + 26 + 16 + 11, (5, 1), B[:9], [17, 17], [7, 2]))
    # a sticky error on entry: nothing is consumed
    add("sticky error on entry", H1, Expect([], hc.EXPECTED_CONTINUATION_FRAME, 0, None, b"", [], []),
        state=State(16384, hc.EXPECTED_CONTINUATION_FRAME, 0, 0))
    add("sticky error on entry, a block pending", frame(CONTINUATION, END_HEADERS, 5, B[4:]),
        Expect([], hc.EXPECTED_CONTINUATION_FOR_STREAM, 0, (5, 1), B[:4], [], [4]),
        state=State(16384, hc.EXPECTED_CONTINUATION_FOR_STREAM, 1, 5 | ES_BIT), carry=B[:4])
    # the reserved bit of a stream id is ignored (section 4.1)
    add("reserved bit in a HEADERS stream id", raw_header(17, HEADERS, END_HEADERS, 0x80000001) + B, Expect(one, 0, 26, None, b"", [17], []))
    add("reserved bit in a CONTINUATION stream id", head + raw_header(12, CONTINUATION, END_HEADERS, 0x80000001) + B[5:],
        Expect(one, 0, 14 + 21, None, b"", [5, 12], []))
    # a block after an error is not listed; the ones before it are
    add("a block after an error is not listed", H1 + frame(CONTINUATION, END_HEADERS, 1, B) + frame(HEADERS, END_HEADERS, 3, B),
        Expect(one, hc.UNEXPECTED_CONTINUATION_FRAME, 52, None, b"", [17], []))
    # other frames between and inside
    add("other frame types are skipped", frame(PING, 0, 0, b"12345678") + H1 + frame(hc.SETTINGS, 0, 0, b"") + frame(0xFF, 0xFF, 9, b"zz"),
        Expect(one, 0, 17 + 26 + 9 + 11, None, b"", [17], []))
    assert len({x.name for x in c}) == len(c)
    return c


def check_expect(case, scan, base=0, carry_at=None):
    """a Scan of the case against its hand-written expectation"""
    e = case.expect
    blocks, held = scan_blocks_bytes(scan, case.data, case.carry, base, carry_at)
    assert blocks == e.blocks, (case.name, blocks)
    assert scan.state.error == e.error and scan.consumed == e.consumed, (case.name, scan.state, scan.consumed)
    assert scan.state.max_frame_size == case.state.max_frame_size
    if e.pending is None:
        assert not scan.state.pending and not scan.open, case.name
    else:
        assert scan.state.pending == 1 and (scan.state.pend_stream & 0x7FFFFFFF, scan.state.pend_stream >> 31) == e.pending, case.name
    assert held == e.held, (case.name, held)
    assert [n for _, n in scan.closed] == e.closed_lens and [n for _, n in scan.open] == e.open_lens, (case.name, scan.closed, scan.open)
    # the blocks tile the closed list
    at = 0
    for _, f, n in scan.blocks:
        assert f == at and n >= 1, case.name
        at += n
    assert at == len(scan.closed), case.name


# ---- generated inputs -------------------------------------------------------------------------------------------
def cut_points(rng, n, calls):
    return sorted(rng.randrange(n + 1) for _ in range(calls - 1)) + [n]


def corrupted_wires(seed=5, n=400):
    """interop wires with one octet of one frame header replaced: (wire, index of the octet)"""
    rng = random.Random(seed)
    wires, _ = hc.interop_connections(seed)
    out = []
    for k in range(n):
        w = bytearray(wires[k % len(wires)][:4000])
        # walk to a random frame header
        heads, pos = [], 0
        while len(w) - pos >= 9:
            heads.append(pos)
            pos += 9 + int.from_bytes(w[pos : pos + 3], "big")
        h = rng.choice(heads)
        i = h + rng.randrange(9)
        w[i] = rng.choice([0, 1, 9, 0x20, 0x28, 0x08, 0xFF, rng.randrange(256)])
        out.append(bytes(w))
    return out


# ---- batches: connections laid out in one blob ---------------------------------------------------------------------
Batch = namedtuple("Batch", "blob off conns blocks frag_off frag_len open_off open_len conn_blk_off conn_frag_off conn_open_off "
                            "conns_out block_bytes")


def expected_batch(items, base=0):
    """items: [(State, data, carry)] -> the call's inputs (blob: `base` filler octets, the connections' bytes end to
    end, then the carries end to end) and, connection by connection from ref_scan_frames, everything the scan and the
    gather give"""
    datas = [bytes(d) for _, d, _ in items]
    n = len(items)
    off = np.zeros(n + 1, np.uint32)
    off[0] = base
    if n:
        off[1:] = base + np.cumsum([len(d) for d in datas])
    hi = int(off[n])
    conns = np.zeros(n, FCONN_DTYPE)
    blob = bytearray(b"\xee" * base + b"".join(datas))
    blocks, fo, fl, oo, ol, block_bytes = [], [], [], [], [], []
    cb, cf, co = [0], [0], [0]
    out = np.zeros(n, FCONN_DTYPE)
    for k, (st, data, carry) in enumerate(items):
        carry_at = len(blob) if st.pending else 0
        if st.pending:
            blob += bytes(carry)
        conns[k] = (st.max_frame_size, st.error, st.pending, st.pend_stream, carry_at, len(carry) if st.pending else 0, 0xDEAD, 0xBEEF)
        s = ref_scan_frames(st, data, carry, int(off[k]), carry_at)
        for sid, f, m in s.blocks:
            blocks.append((k, sid, len(fo) + f, m))
        bb, _ = scan_blocks_bytes(s, data, carry, int(off[k]), carry_at)
        block_bytes += [x[2] for x in bb]
        fo += [a for a, _ in s.closed]
        fl += [m for _, m in s.closed]
        oo += [a for a, _ in s.open]
        ol += [m for _, m in s.open]
        cb.append(len(blocks))
        cf.append(len(fo))
        co.append(len(oo))
        out[k] = (st.max_frame_size, s.state.error, s.state.pending, s.state.pend_stream, carry_at, conns[k]["carry_len"], s.consumed, 0)
    assert hi <= len(blob)
    u = lambda x: np.asarray(x, np.uint32)  # noqa: E731
    return Batch(np.frombuffer(bytes(blob), np.uint8).copy(), off, conns, np.array(blocks, np.uint32).reshape(-1, 4).view(FBLOCK_DTYPE).reshape(-1),
                 u(fo), u(fl), u(oo), u(ol), u(cb), u(cf), u(co), out, block_bytes)
