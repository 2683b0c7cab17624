"""The HTTP/2 frame layer's frame sequences (hpk_h2_read_frames) and a model of its framing.

The generators and the placed error sequences are the ones tests/test_h2.py runs through the library; the stand-alone
host driver (tests/test_host_sanitizers.py) runs the same sequences. ref_read restates what the reference does per
connection with the bytes of one call (crates/loona/src/h2/server.rs:290-390 the deframer's length check and padding
removal, :895-911 the priority block, :1299-1303 and :1349-1417 CONTINUATION gathering) on top of hpack_ref.Decoder:
tests/test_host_sanitizers.py pins it to the hand-written expectations below before it uses it."""

import random

from hpk_util import hpack_ref, load

HEADERS, CONTINUATION, DATA, PRIORITY, SETTINGS, PING = 0x1, 0x9, 0x0, 0x2, 0x4, 0x6
END_STREAM, END_HEADERS, PADDED, PRIO = 0x1, 0x4, 0x8, 0x20

# hpk_h2_error
H2_OK, FRAME_TOO_LARGE, PADDED_FRAME_EMPTY, PADDED_FRAME_TOO_SHORT, PRIORITY_PARSE, HEADERS_INVALID_PRIORITY, \
    EXPECTED_CONTINUATION_FRAME, EXPECTED_CONTINUATION_FOR_STREAM, UNEXPECTED_CONTINUATION_FRAME, COMPRESSION_ERROR = range(10)
H2_NAMES = {None: H2_OK, "FrameTooLarge": 1, "PaddedFrameEmpty": 2, "PaddedFrameTooShort": 3, "ReadAndParse(PrioritySpec)": 4,
            "HeadersInvalidPriority": 5, "ExpectedContinuationFrame": 6, "ExpectedContinuationForStream": 7,
            "UnexpectedContinuationFrame": 8, "HpackDecodingError": 9}


def frame(ftype, flags, stream_id, payload):
    """One frame: RFC 9113 section 4.1 header (24-bit length, type, flags, 31-bit stream id) + payload."""
    n = len(payload)
    return bytes([n >> 16 & 255, n >> 8 & 255, n & 255, ftype, flags]) + (stream_id & 0x7FFFFFFF).to_bytes(4, "big") + \
        bytes(payload)


def header_frames(rng, sid, block, end_stream, max_frame=16384):
    """One header block as HEADERS (+ CONTINUATION) frames: random split, padding, priority."""
    cuts = sorted(rng.sample(range(1, len(block)), min(len(block) - 1, rng.randrange(0, 4)))) if len(block) > 1 else []
    frags = [block[a:b] for a, b in zip([0] + cuts, cuts + [len(block)])]
    out = []
    flags = END_STREAM if end_stream else 0
    first = frags[0]
    if rng.random() < 0.3:  # priority block: 31-bit dependency (never itself) + weight
        first = (sid + 2).to_bytes(4, "big") + bytes([rng.randrange(256)]) + first
        flags |= PRIO
    if rng.random() < 0.3:  # padding: length byte + zeros at the end
        pad = rng.randrange(0, 20)
        first = bytes([pad]) + first + b"\0" * pad
        flags |= PADDED
    assert len(first) <= max_frame
    out.append(frame(HEADERS, flags | (END_HEADERS if len(frags) == 1 else 0), sid, first))
    for i, f in enumerate(frags[1:], 1):
        out.append(frame(CONTINUATION, END_HEADERS if i == len(frags) - 1 else 0, sid, f))
    return out


def other_frame(rng, sid):
    k = rng.randrange(3)
    if k == 0:
        return frame(SETTINGS, 0, 0, b"\0\x03\0\0\0\x64")
    if k == 1:
        return frame(PING, 0, 0, b"12345678")
    body = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 30)))
    return frame(DATA, PADDED, sid, bytes([3]) + body + b"\0\0\0")


def interop_connections(seed=0):
    """(wire bytes per connection, expected [(stream, end_stream, headers)] per connection)."""
    rng = random.Random(seed)
    inter = load("interop.json.gz")
    wires, wants = [], []
    for enc in sorted(inter):
        for story in inter[enc]:
            frames, want = [], []
            for i, c in enumerate(story["cases"]):
                sid = 2 * i + 1
                es = rng.random() < 0.5
                block = bytes.fromhex(c["wire"])
                if not block:
                    continue  # an empty header block is legal but carries nothing to check
                if rng.random() < 0.2:
                    frames.append(other_frame(rng, sid))
                frames += header_frames(rng, sid, block, es)
                want.append((sid, es, [(n.encode(), v.encode()) for n, v in c["headers"]]))
            wires.append(b"".join(frames))
            wants.append(want)
    return wires, wants


BLOCK = bytes.fromhex("828684418cf1e3c2e5f23a6ba0ab90f4ff")  # RFC 7541 C.4.1 (Huffman)
C41 = [(b":method", b"GET"), (b":scheme", b"http"), (b":path", b"/"), (b":authority", b"www.example.com")]

# (the second frame after HEADERS(stream 1, no END_HEADERS), the connection error): read_headers compares the stream
# id before the frame type (server.rs:1391-1397, then 1399-1408)
CHECK_ORDER = [
    # same stream, wrong type: only the type check fails (server.rs:1399-1408)
    (frame(DATA, 0, 1, b"xyz"), "ExpectedContinuationFrame"),
    (frame(HEADERS, END_HEADERS, 1, BLOCK), "ExpectedContinuationFrame"),
    # another stream, any type: the stream check comes first (server.rs:1391-1397)
    (frame(DATA, 0, 3, b"xyz"), "ExpectedContinuationForStream"),
    (frame(CONTINUATION, END_HEADERS, 3, BLOCK[5:]), "ExpectedContinuationForStream"),
    (frame(PING, 0, 0, b"12345678"), "ExpectedContinuationForStream"),
]

# (frames, the connection error, the GOAWAY code)
CONNECTION_ERRORS = [
    ([frame(HEADERS, 0, 1, BLOCK[:5]), frame(CONTINUATION, END_HEADERS, 3, BLOCK[5:])],
     "ExpectedContinuationForStream", "PROTOCOL_ERROR"),
    ([frame(HEADERS, END_HEADERS | PADDED, 1, b"")], "PaddedFrameEmpty", "FRAME_SIZE_ERROR"),
    ([frame(HEADERS, END_HEADERS | PADDED, 1, bytes([40]) + BLOCK)], "PaddedFrameTooShort", "PROTOCOL_ERROR"),
    ([frame(DATA, PADDED, 1, b"")], "PaddedFrameEmpty", "FRAME_SIZE_ERROR"),
    ([frame(HEADERS, END_HEADERS | PRIO, 1, b"\0\0\0\x01\x10" + BLOCK)], "HeadersInvalidPriority", "PROTOCOL_ERROR"),
    ([frame(HEADERS, END_HEADERS | PRIO, 1, b"\0\0")], "ReadAndParse(PrioritySpec)", "PROTOCOL_ERROR"),
    ([frame(CONTINUATION, END_HEADERS, 1, BLOCK)], "UnexpectedContinuationFrame", "PROTOCOL_ERROR"),
    ([frame(DATA, 0, 1, b"x" * 16385)], "FrameTooLarge", "FRAME_SIZE_ERROR"),
]


# ---- the framing model ------------------------------------------------------------------------------------------
class RefConn:
    """one connection: its decoder (hpack_ref.Decoder), a header block waiting for CONTINUATION, the sticky error"""

    def __init__(self, max_frame_size=16384):
        self.dec = hpack_ref.Decoder()
        self.max_frame_size = max_frame_size
        self.pending = None  # (stream, end_stream, fragment bytes so far)
        self.error = H2_OK


def _be31(b):
    return int.from_bytes(b[:4], "big") & 0x7FFFFFFF


def _frames(conn, data):
    """the deframer and the frame loop over one call's bytes -> ([(stream, end_stream, block)], consumed, error)"""
    blocks, pos, err = [], 0, conn.error
    while err == H2_OK and len(data) - pos >= 9:
        length, ftype, flags, sid = int.from_bytes(data[pos : pos + 3], "big"), data[pos + 3], data[pos + 4], _be31(data[pos + 5 :])
        if length > conn.max_frame_size:  # server.rs:318-325
            err = FRAME_TOO_LARGE
            break
        if len(data) - pos - 9 < length:
            break  # the rest of this frame comes with a later call
        p = data[pos + 9 : pos + 9 + length]
        pos += 9 + length
        if ftype in (DATA, HEADERS) and flags & PADDED:  # server.rs:356-382
            if not p:
                err = PADDED_FRAME_EMPTY
                break
            pad, p = p[0], p[1:]
            if len(p) < pad:
                err = PADDED_FRAME_TOO_SHORT
                break
            p = p[: len(p) - pad]
        if conn.pending is not None:  # read_headers' CONTINUATION loop (server.rs:1376-1417)
            psid, pes, frag = conn.pending
            if sid != psid:
                err = EXPECTED_CONTINUATION_FOR_STREAM
                break
            if ftype != CONTINUATION:
                err = EXPECTED_CONTINUATION_FRAME
                break
            conn.pending = (psid, pes, frag + p)
            if flags & END_HEADERS:
                blocks.append((psid, pes, frag + p))
                conn.pending = None
            continue
        if ftype == CONTINUATION:  # server.rs:1299-1303
            err = UNEXPECTED_CONTINUATION_FRAME
            break
        if ftype != HEADERS:
            continue
        if flags & PRIO:  # server.rs:895-911
            if len(p) < 5:
                err = PRIORITY_PARSE
                break
            if _be31(p) == sid:
                err = HEADERS_INVALID_PRIORITY
                break
            p = p[5:]
        es = 1 if flags & END_STREAM else 0
        if flags & END_HEADERS:
            blocks.append((sid, es, p))
        else:
            conn.pending = (sid, es, p)
    return blocks, pos, err


def decode_with_error(dec, wire):
    """hpack_ref.Decoder on one block -> (headers emitted before the first error, DecoderError or None)"""
    out = []
    try:
        dec.decode_with_cb(wire, lambda n, v: out.append((n, v)))
    except hpack_ref.DecoderError as e:
        return out, e
    return out, None


def ref_read(conns, chunks):
    """one hpk_h2_read_frames call -> (conn_error per connection, conn_consumed per connection, [(conn, stream,
    end_stream, skipped, headers, DecoderError or None)] in the call's block order). A decoding error is the
    connection's COMPRESSION_ERROR and comes before a framing error of the same call; the connection's later blocks of
    the call are skipped (the reference never decodes them)."""
    errors, consumed, out = [], [], []
    for c, (conn, data) in enumerate(zip(conns, chunks)):
        blocks, pos, ferr = _frames(conn, bytes(data))
        consumed.append(pos)
        dead = False
        for sid, es, wire in blocks:
            if dead:
                out.append((c, sid, es, 1, [], None))
                continue
            headers, err = decode_with_error(conn.dec, wire)
            out.append((c, sid, es, 0, headers, err))
            if err is not None:
                dead = True
        conn.error = COMPRESSION_ERROR if dead else ferr
        errors.append(conn.error)
    return errors, consumed, out
