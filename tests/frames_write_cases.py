"""The frame write's cases (hpk_write_frames, hpk_write_frames_cpu, hpk_h2_write_headers) and a model of it.

ref_write_frames restates the reference's header loop of send_data_maybe (crates/loona/src/h2/server.rs:470-508: a
piece strictly longer than the peer's max frame size goes as that many octets without flags, HEADERS first and
CONTINUATION after; the last piece, empty only for the empty block, carries END_HEADERS) with Frame::write_into's
9-octet header (crates/loona-h2/src/lib.rs:413-422) in front of each piece. The stream word's bit 31 asks for
END_STREAM on the HEADERS frame, hpk_fblock's convention. tests/test_frames_write_cases.py pins it to the hand-written
octets of placed() and to frames_cases.ref_scan_frames before the emulation and the GPU tests use it.

placed() is written from RFC 9113 (section 4.1 the frame header, 4.2 the size limit, 6.2 HEADERS, 6.10 CONTINUATION)
and the cited lines, never from the model."""

from collections import namedtuple

import numpy as np

from hpk_util import load

ES_BIT = 0x80000000
MAX_FRAME_TOP = 0xFFFFFF
HPK_MAX_OFFSET = 0xFFFFFFDF
HPK_OK, HPK_BAD_OFFSETS = 0, 5


def frame_count(length, m):
    return max(1, -(-length // m))


def wire_len(length, m):
    return length + 9 * frame_count(length, m)


def ref_write_frames(block, stream_word, m):
    """one block's octets on the wire"""
    block = bytes(block)
    assert 1 <= m <= MAX_FRAME_TOP
    out, piece, first = [], block, True
    sid = (stream_word & 0x7FFFFFFF).to_bytes(4, "big")
    while True:  # 'queue_header_frames
        if len(piece) > m:
            written, piece = piece[:m], piece[m:]
            flags, last = 0, False
        else:
            written, flags, last = piece, 0x4, True
        if first and stream_word & ES_BIT:
            flags |= 0x1
        out.append(len(written).to_bytes(3, "big") + bytes([0x1 if first else 0x9, flags]) + sid + written)
        first = False
        if last:
            return b"".join(out)


Case = namedtuple("Case", "name block stream_word max_frame wire frames")


def H(hexes):
    return bytes.fromhex(hexes.replace(" ", ""))


def placed():
    """blocks with their hand-written wire octets and frame counts"""
    c = []

    def add(name, block, word, m, wire, frames):
        c.append(Case(name, bytes(block), word, m, bytes(wire), frames))

    add("L = 0", b"", 1, 16384, H("000000 01 04 00000001"), 1)
    add("L = 0, M = 1", b"", 3, 1, H("000000 01 04 00000003"), 1)
    add("L = 1, M = 1", b"a", 1, 1, H("000001 01 04 00000001") + b"a", 1)
    add("L = 2, M = 1", b"ab", 1, 1, H("000001 01 00 00000001") + b"a" + H("000001 09 04 00000001") + b"b", 2)
    add("L = M (5)", b"abcde", 3, 5, H("000005 01 04 00000003") + b"abcde", 1)
    add("L = M + 1", b"abcdef", 3, 5, H("000005 01 00 00000003") + b"abcde" + H("000001 09 04 00000003") + b"f", 2)
    add("L = 2M - 1", b"abcdefghi", 3, 5, H("000005 01 00 00000003") + b"abcde" + H("000004 09 04 00000003") + b"fghi", 2)
    add("L = 2M", b"abcdefghij", 3, 5, H("000005 01 00 00000003") + b"abcde" + H("000005 09 04 00000003") + b"fghij", 2)
    add("L = 2M + 1", b"abcdefghijk", 3, 5,
        H("000005 01 00 00000003") + b"abcde" + H("000005 09 00 00000003") + b"fghij" + H("000001 09 04 00000003") + b"k", 3)
    add("END_STREAM, three frames", b"abcde", 5 | ES_BIT, 2,
        H("000002 01 01 00000005") + b"ab" + H("000002 09 00 00000005") + b"cd" + H("000001 09 04 00000005") + b"e", 3)
    add("END_STREAM, one frame", b"xy", 7 | ES_BIT, 16384, H("000002 01 05 00000007") + b"xy", 1)
    add("END_STREAM, the empty block", b"", 9 | ES_BIT, 16384, H("000000 01 05 00000009"), 1)
    add("stream id 0x7FFFFFFF", b"x", 0x7FFFFFFF, 16384, H("000001 01 04 7fffffff") + b"x", 1)
    add("stream id 0x7FFFFFFF with END_STREAM", b"x", 0xFFFFFFFF, 16384, H("000001 01 05 7fffffff") + b"x", 1)
    add("M = 0xFFFFFF, a short block", b"hello", 1, 0xFFFFFF, H("000005 01 04 00000001") + b"hello", 1)
    add("a length above 255", bytes(range(256)) + b"\x01\x02", 0x01020304, 300, H("000102 01 04 01020304") + bytes(range(256)) + b"\x01\x02", 1)
    assert len({x.name for x in c}) == len(c)
    return c


def interop_blocks(limit=None):
    """the interop corpus' header blocks (tests/golden/interop.json.gz), in a fixed order"""
    inter = load("interop.json.gz")
    out = []
    for enc in sorted(inter):
        for story in inter[enc]:
            for case in story["cases"]:
                out.append(bytes.fromhex(case["wire"]))
                if limit is not None and len(out) >= limit:
                    return out
    return out


Batch = namedtuple("Batch", "blob block_off stream_id max_frame wire wire_off status total")


def expected_batch(items, base=0):
    """items: [(block bytes, stream word, max_frame)] -> the call's inputs (blob: `base` filler octets, then the
    blocks end to end) and what the call gives, block by block from ref_write_frames. An item whose max_frame is 0 or
    above 0xFFFFFF is void: no octets, HPK_BAD_OFFSETS."""
    n = len(items)
    block_off = np.zeros(n + 1, np.uint32)
    block_off[0] = base
    if n:
        block_off[1:] = base + np.cumsum([len(b) for b, _, _ in items])
    blob = np.frombuffer(b"\xee" * base + b"".join(bytes(b) for b, _, _ in items) or b"\0", np.uint8).copy()[: int(block_off[n])]
    sid, mf = u32([w for _, w, _ in items]), u32([m for _, _, m in items])
    wire, wire_off, status, total = expected_from(blob, blob.size, block_off, sid, mf)
    return Batch(blob, block_off, sid, mf, wire, wire_off, status, total)


def u32(x):
    return np.asarray(x, np.uint32)


def expected_from(blob, cap, block_off, sid, mf):
    """what a device-pointer call gives for these arrays as they lie -> (wire, wire_off, status, total): a block whose
    offsets decrease or pass cap, or whose max_frame is 0 or above 0xFFFFFF, is void (no octets, HPK_BAD_OFFSETS) and
    voids no other; a total past HPK_MAX_OFFSET voids all"""
    n = len(sid)
    wires, status = [], []
    for b in range(n):
        a, e, m = int(block_off[b]), int(block_off[b + 1]), int(mf[b])
        ok = a <= e <= cap and 1 <= m <= MAX_FRAME_TOP
        wires.append(ref_write_frames(bytes(blob[a:e]), int(sid[b]), m) if ok else b"")
        status.append(HPK_OK if ok else HPK_BAD_OFFSETS)
    wire_off = np.zeros(n + 1, np.int64)
    if n:
        wire_off[1:] = np.cumsum([len(x) for x in wires])
    total = int(wire_off[n])
    assert total <= HPK_MAX_OFFSET
    return np.frombuffer(b"".join(wires), np.uint8).copy(), wire_off.astype(np.uint32), np.asarray(status, np.uint8), total
