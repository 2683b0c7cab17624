"""HTTP/2 header reading across many connections with one Huffman batch.

Mirrors what loona's h2 server does per connection before it hands a header block to its HPACK
decoder — the deframer (crates/loona/src/h2/server.rs:290-390: frame length check, padding), the
HEADERS priority block (server.rs:895-911) and read_headers' CONTINUATION gathering
(server.rs:1349-1417, 1619-1638) — over the bytes of MANY connections at once, then decodes every
complete header block of every connection with one hpk_hdec_decode_blocks call (include/hpk.h
hpk_h2_read_frames):

    conns = [Connection() for _ in range(n)]
    res = read_frames(conns, [bytes_of_conn0, bytes_of_conn1, ...], codec)   # codec=None: CPU batch
    res.blocks    -> [(conn, stream_id, end_stream, headers | DecoderError | None (skipped))]
    res.errors    -> per connection: H2Error name or None; res.consumed -> bytes used per connection

A connection keeps a HEADERS block whose CONTINUATION frames have not all arrived, and its HPACK
dynamic table, between calls; its first error ends it (the reference sends GOAWAY with
H2Error.code(name)).
"""

from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .hpack import _error

ERRORS = {  # hpk_h2_error -> the reference's H2ConnectionError variant
    1: "FrameTooLarge",
    2: "PaddedFrameEmpty",
    3: "PaddedFrameTooShort",
    4: "ReadAndParse(PrioritySpec)",
    5: "HeadersInvalidPriority",
    6: "ExpectedContinuationFrame",
    7: "ExpectedContinuationForStream",
    8: "UnexpectedContinuationFrame",
    9: "HpackDecodingError",
}
CODES = {0x1: "PROTOCOL_ERROR", 0x6: "FRAME_SIZE_ERROR", 0x9: "COMPRESSION_ERROR", 0x0: "NO_ERROR"}


def error_code(name):
    """RFC 9113 §7 error code name the reference's GOAWAY carries for a connection error."""
    inv = {v: k for k, v in ERRORS.items()}
    return CODES[_lib.lib().hpk_h2_error_code(inv[name] if name else 0)]


class Connection:
    """One connection's header-reading state (hpk_h2conn): HPACK decoder + pending CONTINUATION."""

    def __init__(self, max_frame_size: int = 16384):
        self._L = _lib.lib()
        self._h = self._L.hpk_h2conn_create()
        if not self._h:
            raise MemoryError("hpk_h2conn_create")
        if max_frame_size != 16384:
            _lib.check(self._L.hpk_h2conn_set_max_frame_size(self._h, max_frame_size), "hpk_h2conn_set_max_frame_size")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.hpk_h2conn_destroy(h)

    @property
    def error(self):
        e = self._L.hpk_h2conn_error(self._h)
        return ERRORS.get(e) if e else None


class Result:
    def __init__(self, blocks, errors, consumed):
        self.blocks, self.errors, self.consumed = blocks, errors, consumed


class Arena:
    """buffet's buffer arena (hpk_arena_create: one anonymous mmap of num_bufs x buf_size, page-locked
    when pin): .view is a writable numpy view of it; read_frames_in() decodes frames in place."""

    def __init__(self, num_bufs=65536, buf_size=4096, pin=True):
        self._L = _lib.lib()
        self._h = self._L.hpk_arena_create(num_bufs, buf_size, 1 if pin else 0)
        if not self._h:
            raise RuntimeError(f"hpk_arena_create failed: {_lib.last_error()}")
        n = self._L.hpk_arena_len(self._h)
        self.base = self._L.hpk_arena_base(self._h)
        self.view = np.ctypeslib.as_array((ctypes.c_uint8 * n).from_address(self.base))

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self.view = None
            self._L.hpk_arena_destroy(h)

    def __del__(self):
        self.close()


def read_frames_in(conns, arena, offsets, codec=None) -> Result:
    """read_frames on bytes already in an Arena: connection c's bytes are
    arena.view[offsets[c] : offsets[c+1]] (no copy on the way in)."""
    off32 = np.ascontiguousarray(offsets, dtype=np.uint32)
    return _read(conns, arena.base, off32, codec)


def read_frames(conns, chunks, codec=None) -> Result:
    """Frames received on each connection (chunks[c] = bytes for conns[c]) -> decoded header blocks."""
    L = _lib.lib()
    n = len(conns)
    if len(chunks) != n:
        raise ValueError("one byte chunk per connection")
    off = np.zeros(n + 1, np.int64)
    np.cumsum([len(c) for c in chunks], out=off[1:])
    if off[-1] >= 2**32:
        raise ValueError("the bytes of one call must stay below 4 GiB")
    blob = np.frombuffer(b"".join(bytes(c) for c in chunks) or b"\0", dtype=np.uint8).copy()
    return _read(conns, blob.ctypes.data, off.astype(np.uint32), codec)


def _read(conns, base, off32, codec):
    L = _lib.lib()
    n = len(conns)
    hs = (ctypes.c_void_p * max(n, 1))(*[c._h for c in conns])
    out = _lib.H2Out()
    ctx = codec._h if codec is not None else None
    _lib.check(L.hpk_h2_read_frames(ctx, hs, base, off32.ctypes.data, n, ctypes.byref(out)),
               "hpk_h2_read_frames")
    try:
        arena = ctypes.string_at(out.hb.arena, out.hb.arena_len) if out.hb.arena_len else b""
        blocks = []
        for b in range(out.hb.n_blocks):
            m = out.blocks[b]
            if m.skipped:
                val = None
            else:
                r = out.hb.blocks[b]
                hl = []
                for j in range(r.first_header, r.first_header + r.n_headers):
                    h = out.hb.headers[j]
                    hl.append((arena[h.name_off : h.name_off + h.name_len],
                               arena[h.value_off : h.value_off + h.value_len]))
                val = hl if r.error == 0 else _error(r.error, r.detail)
            blocks.append((m.conn, m.stream_id, bool(m.end_stream), val))
        errors = [ERRORS.get(out.conn_error[c]) if out.conn_error[c] else None for c in range(n)]
        consumed = [out.conn_consumed[c] for c in range(n)]
        return Result(blocks, errors, consumed)
    finally:
        L.hpk_h2_out_free(ctypes.byref(out))


def frame(ftype: int, flags: int, stream_id: int, payload: bytes) -> bytes:
    """One frame: RFC 9113 §4.1 header (24-bit length, type, flags, 31-bit stream id) + payload."""
    n = len(payload)
    return bytes([n >> 16 & 255, n >> 8 & 255, n & 255, ftype, flags]) + (stream_id & 0x7FFFFFFF).to_bytes(4, "big") + \
        bytes(payload)


def write_frames_cpu(blocks, block_off, stream_ids, max_frame_sizes, out_cap=None):
    """hpk_write_frames_cpu: numpy in -> (wire octets, wire_off, status, return code). Block b =
    blocks[block_off[b] : block_off[b+1]] becomes one HEADERS frame and the CONTINUATION frames that
    max_frame_sizes[b] demands (server.rs:470-508), stream_ids[b]'s bit 31 asking for END_STREAM. out_cap defaults
    to what the blocks need. The code is returned, not raised: HPK_E_NOSPACE (-2) still fills the arrays."""
    L = _lib.lib()
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8)
    block_off = np.ascontiguousarray(block_off, dtype=np.uint32)
    sid = np.ascontiguousarray(stream_ids, dtype=np.uint32)
    mf = np.ascontiguousarray(max_frame_sizes, dtype=np.uint32)
    n = len(block_off) - 1
    if len(sid) != n or len(mf) != n:
        raise ValueError("one stream id and one frame size per block")
    if out_cap is None:
        lens = np.diff(block_off.astype(np.int64))
        m = np.maximum(mf.astype(np.int64), 1)
        out_cap = int((np.maximum(lens, 0) + 9 * np.maximum(-(-lens // m), 1)).sum()) if n > 0 else 0
    out = np.full(max(int(out_cap), 1), 0xA5, dtype=np.uint8)
    wire_off = np.zeros(n + 1, dtype=np.uint32)
    status = np.zeros(max(n, 1), dtype=np.uint8)
    data = blocks if blocks.size else np.zeros(1, dtype=np.uint8)
    rc = L.hpk_write_frames_cpu(data.ctypes.data, blocks.size, block_off.ctypes.data, n, sid.ctypes.data if n else None,
                                mf.ctypes.data if n else None, out.ctypes.data, int(out_cap), wire_off.ctypes.data,
                                status.ctypes.data if n else None)
    return out[: int(out_cap)], wire_off, status[:n], rc


def write_headers(encoders, header_lists, stream_ids, max_frame_sizes, codec=None):
    """Many responses' headers -> the octets to send, one bytes object per block (hpk_h2_write_headers):
    header_lists[b] = [(name, value)] is encoded with encoders[b] (hpack.Encoder; the blocks of one encoder in list
    order, as hpack.encode_blocks) and framed for stream stream_ids[b] (bit 31: END_STREAM on the HEADERS frame) as
    one HEADERS frame and the CONTINUATION frames max_frame_sizes[b], the peer's SETTINGS_MAX_FRAME_SIZE, demands
    (server.rs:470-508). A frame size of 0 or above 0xFFFFFF raises before any encoder is touched. codec=None: all
    on the host; with a codec the encode goes as it selects, and codec.set_frame_write('device') frames on the
    device too."""
    L = _lib.lib()
    n = len(encoders)
    if not (len(header_lists) == len(stream_ids) == len(max_frame_sizes) == n):
        raise ValueError("one header list, stream id and frame size per encoder")
    parts, off, hoff = [], [0], [0]
    for headers in header_lists:
        for name, value in headers:
            for x in (name, value):
                parts.append(bytes(x))
                off.append(off[-1] + len(x))
        hoff.append(hoff[-1] + len(headers))
    if off[-1] >= 2**32:
        raise ValueError("header fields of one call must stay below 4 GiB")
    fields = np.frombuffer(b"".join(parts) or b"\0", dtype=np.uint8).copy()
    off32 = np.asarray(off, dtype=np.uint32)
    hoff32 = np.asarray(hoff, dtype=np.uint32)
    sid = np.asarray(list(stream_ids) or [0], dtype=np.uint32)
    mf = np.asarray(list(max_frame_sizes) or [1], dtype=np.uint32)
    encs = (ctypes.c_void_p * max(n, 1))(*[e._h for e in encoders])
    out = _lib.HencOut()
    ctx = codec._h if codec is not None else None
    _lib.check(L.hpk_h2_write_headers(ctx, encs, fields.ctypes.data, off32.ctypes.data, hoff32.ctypes.data, n, sid.ctypes.data,
                                      mf.ctypes.data, ctypes.byref(out)), "hpk_h2_write_headers")
    try:
        data = ctypes.string_at(out.bytes, out.len) if out.len else b""
        return [data[out.block_off[b] : out.block_off[b + 1]] for b in range(n)]
    finally:
        L.hpk_henc_out_free(ctypes.byref(out))
