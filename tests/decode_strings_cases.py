"""Cases for the packed string-literal decode (hpk_decode_strings_packed), shared by test_decode_strings_cases.py
(CPU: expected() agrees with hpack_ref.decode_string, a placed case reaches the cut or edge it claims),
test_strparse_emulation.py (the parse step on the host) and test_gpu_decode_strings.py (the device result, byte
for byte).

A batch is (blob, str_off, str_end): the input bytes and one window [str_off[i], str_end[i]) per string. The
expected answer never comes from the code under test: expected() takes the prefix from hpack_ref.decode_integer,
applies decode_string's length check (decoder.rs:138), and takes a Huffman payload's bytes and status from the C
oracle (which keeps the bytes decoded before an error; hpack_ref.decode_string raises without them).
test_decode_strings_cases.py proves that this model is hpack_ref.decode_string window by window."""

import collections

import numpy as np

from hpk_util import hpack_ref, load, oracle_decode_batch, oracle_encode, pack
from loona_amd import _lib

# the per-string status values as the binding names them (test_decode_strings_host.py pins their numbers)
OK, BAD_OFFSETS = _lib.HPK_OK, _lib.HPK_BAD_OFFSETS
TOO_MANY, INT_SHORT, STR_SHORT = (_lib.HPK_PREFIX_TOO_MANY_OCTETS, _lib.HPK_PREFIX_NOT_ENOUGH_OCTETS,
                                  _lib.HPK_STRING_NOT_ENOUGH_OCTETS)

Expected = collections.namedtuple("Expected", "out_off out_len consumed status flat huff pay_off pay_len")
Batch = collections.namedtuple("Batch", "blob str_off str_end")


def frame(payload, huff):
    """a payload behind its 7-bit-prefix length (hpack_ref.encode_integer), 0x80 set for the Huffman form"""
    return bytes(hpack_ref.encode_integer(len(payload), 7, 0x80 if huff else 0)) + bytes(payload)


def frame_plain(s, huff):
    """the string-literal representation of plaintext s: raw, or its Huffman coding (the C oracle's)"""
    return frame(oracle_encode(s) if huff else s, huff)


def batch_of(windows, tail=b""):
    """the windows end to end (the mirror form's layout) -> Batch; `tail`: bytes after the last window"""
    blob, off = pack(list(windows) + [tail])
    off = off.astype(np.int64)
    return Batch(blob, off[:-2], off[1:-1])


def to_end(b):
    """the same strings with every window extended to the blob's end (the reference's "rest of the block")"""
    return Batch(b.blob, b.str_off, np.full(len(b.str_off), b.blob.size, np.int64))


def parse(head, wlen):
    """decode_string's front half on one window by hpack_ref.decode_integer -> (status, H, prefix octets, length).
    head: the window's first min(wlen, 5) octets (decode_integer never looks further); wlen: the window's bytes."""
    try:
        ln, used = hpack_ref.decode_integer(head, 7)
    except hpack_ref.DecoderError as e:
        assert e.kind == "IntegerDecodingError"
        return {"TooManyOctets": TOO_MANY, "NotEnoughOctets": INT_SHORT}[e.detail], 0, 0, 0
    if used + ln > wlen:  # decoder.rs:138
        return STR_SHORT, 0, 0, 0
    return OK, head[0] >> 7, used, ln


def expected(b, in_cap=None):
    """The answer to a batch. A window with str_off > str_end or str_end > in_cap is void (BAD_OFFSETS)."""
    blob = np.asarray(b.blob, np.uint8)
    in_cap = blob.size if in_cap is None else in_cap
    n = len(b.str_off)
    status = np.zeros(n, np.uint8)
    huff = np.zeros(n, bool)
    pay_off = np.zeros(n, np.int64)
    pay_len = np.zeros(n, np.int64)
    consumed = np.zeros(n, np.int64)
    raw = blob.tobytes()
    for i, (a, e) in enumerate(zip(np.asarray(b.str_off).tolist(), np.asarray(b.str_end).tolist())):
        if a > e or e > in_cap:
            status[i] = BAD_OFFSETS
            continue
        st, h, used, ln = parse(raw[a : min(e, a + 5)], e - a)
        status[i] = st
        if st == OK:
            huff[i], pay_off[i], pay_len[i], consumed[i] = bool(h), a + used, ln, used + ln
    out_len = np.where(huff, 0, pay_len)
    pieces = [None] * n
    hi = np.nonzero(huff)[0]
    if hi.size:  # every Huffman payload through the C oracle in one call
        hb, ho = pack([raw[pay_off[i] : pay_off[i] + pay_len[i]] for i in hi])
        ob, oo, ol, st = oracle_decode_batch(hb, ho)
        for j, i in enumerate(hi):
            status[i] = st[j]
            out_len[i] = ol[j]
            pieces[i] = ob[int(oo[j]) : int(oo[j]) + int(ol[j])]
    for i in np.nonzero(~huff & (pay_len > 0))[0]:
        pieces[i] = blob[pay_off[i] : pay_off[i] + pay_len[i]]
    out_off = np.zeros(n + 1, np.int64)
    np.cumsum(out_len, out=out_off[1:])
    live = [p for p in pieces if p is not None and len(p)]
    flat = np.concatenate(live) if live else np.zeros(0, np.uint8)
    assert flat.size == out_off[-1]
    return Expected(out_off, out_len.astype(np.int64), consumed, status, flat, huff, pay_off, pay_len)


# ---- prefix shapes --------------------------------------------------------------------------------------

PREFIX_VALUES = (0, 126, 127, 128, 254, 255, 127 + 2**7, 127 + 2**14, 127 + 2**21, 127 + 2**28 - 1)
FIVE_BIT = b"012aceiost"  # codes of 5 bits: n of them are a Huffman payload of ceil(5 n / 8) bytes


def payload_of(nbytes, huff, seed):
    """nbytes of payload: uniform bytes (raw), or the Huffman coding of 5-bit symbols that fills nbytes exactly"""
    rng = np.random.default_rng(31000 + seed)
    if not huff:
        return rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes()
    s = bytes(rng.choice(np.frombuffer(FIVE_BIT, np.uint8), 8 * nbytes // 5).astype(np.uint8))
    p = oracle_encode(s)
    assert len(p) == nbytes
    return p


def prefix_shapes(max_payload=16511):
    """Windows around every edge of the prefix and the length check -> list of (what, window bytes). For each
    value of PREFIX_VALUES and both H values: the integer cut at every window length from 0 up to its own length;
    where the payload is at most max_payload bytes, the string with length == window, length == window + 1 (one
    byte short) and three trailing bytes. Then a 5th octet with the continuation bit (alone, and with bytes after
    it), the largest 5-octet value, and padded non-canonical integers with their payloads."""
    out = []
    for v in PREFIX_VALUES:
        for h in (0, 1):
            octets = bytes(hpack_ref.encode_integer(v, 7, 0x80 if h else 0))
            for k in range(len(octets) + 1):
                out.append((f"value {v} H{h} cut at {k}", octets[:k]))
            if v <= max_payload:
                p = payload_of(v, h, v)
                out.append((f"value {v} H{h} exact", octets + p))
                if v:
                    out.append((f"value {v} H{h} one short", octets + p[:-1]))
                out.append((f"value {v} H{h} trailing", octets + p + b"\xff\x80\x7f"))
    for h in (0x00, 0x80):
        lead = bytes((0x7F | h,))
        out.append((f"5th octet continues H{h >> 7}", lead + b"\xff\xff\xff\xff"))
        out.append((f"5th octet continues H{h >> 7}, more bytes", lead + b"\x80\x80\x80\x80\x00\x00\x01"))
        out.append((f"5th octet ends H{h >> 7}", lead + b"\xff\xff\xff\x7f" + b"ab"))
        for pad, v in ((b"\x80\x00", 127), (b"\x80\x80\x00", 127), (b"\x80\x80\x80\x00", 127), (b"\x81\x80\x00", 128),
                       (b"\x83\x80\x80\x00", 130)):
            p = payload_of(v, h >> 7, v + len(pad))
            out.append((f"padded {pad.hex()} H{h >> 7}", lead + pad + p))
            out.append((f"padded {pad.hex()} H{h >> 7} one short", lead + pad + p[:-1]))
            out.append((f"padded {pad.hex()} H{h >> 7} trailing", lead + pad + p + b"\xff"))
    return out


# ---- string sets ------------------------------------------------------------------------------------------

RFC_C_LITERALS = [b"www.example.com", b"no-cache", b"custom-key", b"custom-value", b"302", b"private",
                  b"Mon, 21 Oct 2013 20:13:21 GMT", b"https://www.example.com", b"Mon, 21 Oct 2013 20:13:22 GMT", b"gzip",
                  b"foo=ASDJKHQKBZXOQWEOPIUAXQWEOIU; max-age=3600; version=1", b"307"]


def interop_strings(k=2000):
    """the first k header names and values of the interop corpus (plaintext)"""
    inter = load("interop.json.gz")
    out = []
    for enc in sorted(inter):
        for story in inter[enc]:
            for c in story["cases"]:
                for name, value in c["headers"]:
                    out.append(name.encode())
                    out.append(value.encode())
                    if len(out) >= k:
                        return out[:k]
    return out


def round_trip_strings():
    """RFC App. C literals, ~2k interop header strings, empty strings and 5 % uniform-byte strings (which AUTO
    leaves raw)"""
    rng = np.random.default_rng(32000)
    strs = list(RFC_C_LITERALS) + interop_strings(2000) + [b""] * 20
    for _ in range(len(strs) // 20):
        strs.append(rng.integers(0, 256, int(rng.integers(1, 80)), dtype=np.uint8).tobytes())
    order = rng.permutation(len(strs))
    return [strs[i] for i in order]


def error_vectors(k=200):
    """k of the Huffman error vectors, every reference error among them -> list of (payload, status)"""
    vecs = [(bytes.fromhex(v["in"]), v["status"]) for v in load("error_vectors.json")["vectors"] if v["status"] != 0]
    by = {1: [], 2: [], 3: []}
    for p, s in vecs:
        by[s].append((p, s))
    assert all(by.values())
    out = []
    while len(out) < k and any(by.values()):
        for s in (1, 2, 3):
            if by[s] and len(out) < k:
                out.append(by[s].pop(0))
    return out


# ---- placed pack cases ------------------------------------------------------------------------------------

def alternating(n=600, seed=0):
    """raw and Huffman strings of 1..7 decoded bytes in turn: every 16-byte chunk of the output mixes both sources"""
    rng = np.random.default_rng(33000 + seed)
    wins = []
    for i in range(n):
        s = bytes(rng.choice(np.frombuffer(FIVE_BIT, np.uint8), int(rng.integers(1, 8))).astype(np.uint8))
        wins.append(frame_plain(s, i % 2 == 1))
    return batch_of(wins)


def empties_then_one(lds_literals, seed=0):
    """a short string, more than lds_literals consecutive empty or void strings, then non-empty ones"""
    wins = [frame(b"ab", False)]
    kinds = (b"\x00", b"\x80", b"", b"\x7f", b"\x05ab")  # empty raw, empty Huffman, no octet, cut integer, short payload
    wins += [kinds[i % len(kinds)] for i in range(lds_literals + 37)]
    wins += [frame_plain(b"custom-value", True), frame(b"xyz", False)]
    return batch_of(wins)


def long_raw(tile_bytes, seed=0):
    """a raw string of tile_bytes + 17 bytes among short ones of both forms"""
    rng = np.random.default_rng(34000 + seed)
    wins = [frame_plain(b"custom-key", True), frame(b"q", False)]
    wins.append(frame(rng.integers(0, 256, tile_bytes + 17, dtype=np.uint8).tobytes(), False))
    wins += [frame_plain(b"no-cache", True), frame(b"tail", False)]
    return batch_of(wins)


def sizes_batch(seed=0):
    """Huffman payloads of 63, 64 and 113 encoded bytes and one of 64 KiB (the decode's long and huge phases),
    among short strings of both forms"""
    rng = np.random.default_rng(35000 + seed)
    wins = []
    for nbytes in (63, 64, 113, 65536):
        for _ in range(3):
            s = bytes(rng.choice(np.frombuffer(FIVE_BIT, np.uint8), int(rng.integers(1, 12))).astype(np.uint8))
            wins.append(frame_plain(s, bool(rng.integers(0, 2))))
        wins.append(frame(payload_of(nbytes, True, nbytes), True))
    wins.append(frame(b"end", False))
    return batch_of(wins)


def mixed_batch(n, seed, raw_share=0.3, hi=60):
    """n header-like strings of 0..hi bytes, raw_share of them raw"""
    rng = np.random.default_rng(seed)
    chars = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789-./=; ", np.uint8)
    lens = rng.integers(0, hi + 1, n)
    raw = rng.random(n) < raw_share
    strs = [bytes(rng.choice(chars, int(k)).astype(np.uint8)) for k in lens]
    return batch_of([frame_plain(s, not r) for s, r in zip(strs, raw)]), strs
