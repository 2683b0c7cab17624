"""The header-block apply's reference model and its placed cases (hpk_apply_blocks, loona_amd/csrc/hpk_blkapply.h).

ref_apply is a Python model of the call: per decoder a table of (name, value) entries, newest first, and the
decoder's blocks in order; per block blocks_scan_cases.ref_scan's records and the block's strings decoded by
hpack_ref, applied in the order hpk_hdec.cpp's apply_block states; and the deferral rule for a given ring size
(lim = min(ring, the table's cap)). Names and values are bytes here, where the library moves references into an
arena; the tests resolve the library's references before they compare. tests/test_blocks_apply_cases.py pins
ref_apply to hpack_ref.Decoder; the emulation and the GPU tests compare the real step with it."""

import blocks_scan_cases as bc
from hpk_util import hpack_ref

# hpk_block_error values the apply adds to the scan's
E_OK, E_OOB, E_HUFFMAN, E_INVALID_MAX, E_SU_AT_END, E_DEFERRED = 0, 1, 7, 8, 9, 10

_KIND = {1: ("HeaderIndexOutOfBounds", None), 2: ("IntegerDecodingError", "TooManyOctets"),
         4: ("IntegerDecodingError", "NotEnoughOctets"), 6: ("StringDecodingError", "NotEnoughOctets"),
         8: ("InvalidMaxDynamicSize", None), 9: ("SizeUpdateAtEnd", None)}


def as_decoder_error(error, detail):
    """(hpk_block_error, detail) as hpack_ref.DecoderError's (kind, detail)"""
    if error == E_HUFFMAN:
        return ("StringDecodingError", ("HuffmanDecoderError", detail))
    return _KIND[error]


def static_table():
    return hpack_ref.Decoder().static


class Table:
    """one decoder's dynamic table as hpk_dtab states it: entries newest first, cap the records it may grow into"""

    def __init__(self, entries=(), max_size=4096, max_allowed=None, cap=None):
        self.entries = [(bytes(n), bytes(v)) for n, v in entries]
        self.max_size = max_size
        self.max_allowed = max_allowed
        self.cap = cap
        self.size = sum(len(n) + len(v) + 32 for n, v in self.entries)

    def copy(self):
        return Table(self.entries, self.max_size, self.max_allowed, self.cap)

    def evict(self, incoming=0):
        while self.size + incoming > self.max_size and self.entries:
            n, v = self.entries.pop()
            self.size -= len(n) + len(v) + 32

    def insert(self, name, value):
        sz = len(name) + len(value) + 32
        if sz > self.max_size:  # empties the table and adds nothing
            self.entries, self.size = [], 0
            return
        self.evict(sz)
        self.entries.insert(0, (name, value))
        self.size += sz

    def lookup(self, index, static):
        if index == 0:
            return None
        if index <= len(static):
            return static[index - 1]
        di = index - 1 - len(static)
        return self.entries[di] if di < len(self.entries) else None


def decode_strings(block, strings):
    """the listed strings of a block as hpk_decode_strings_packed leaves them: [(status, bytes)]"""
    out = []
    for a, e in strings:
        ln, c = hpack_ref.decode_integer(block[a:e], 7)
        raw = bytes(block[a + c : e])
        assert c + ln == e - a
        out.append(hpack_ref.huffman_decode(raw) if block[a] & 128 else (0, raw))
    return out


def ref_apply_block(tab, fields, strs, static):
    """apply_block over the device scan's records: -> (headers, error, detail), the headers those emitted before the first error"""
    out = []
    last_update = False
    for f in fields:
        last_update = f.kind == bc.SIZE_UPDATE
        if f.err and f.err_stage == bc.ST_INDEX:
            return out, f.err, 0
        if f.kind == bc.INDEXED:
            h = tab.lookup(f.index, static)
            if h is None:
                return out, E_OOB, 0
            out.append(h)
            continue
        if f.kind == bc.SIZE_UPDATE:
            if tab.max_allowed is not None and f.index > tab.max_allowed:
                return out, E_INVALID_MAX, 0
            tab.max_size = f.index
            tab.evict()
            continue
        s = f.str
        if f.index == 0:
            if f.err and f.err_stage == bc.ST_NAME:
                return out, f.err, 0
            st, name = strs[s]
            if st:
                return out, E_HUFFMAN, st
            s += 1
        else:
            h = tab.lookup(f.index, static)
            if h is None:
                return out, E_OOB, 0
            name = h[0]
        if f.err and f.err_stage == bc.ST_VALUE:
            return out, f.err, 0
        st, value = strs[s]
        if st:
            return out, E_HUFFMAN, st
        out.append((name, value))
        if f.kind == bc.LIT_INCR:
            tab.insert(name, value)
    if last_update:
        return out, E_SU_AT_END, 0
    return out, E_OK, 0


def ref_apply(decoders, ring):
    """decoders: [(Table, [block])]. Applies each decoder's blocks in order, the tables changed in place, with the
    call's deferral rule for a ring of `ring` records -> [(results, applied)] per decoder, results one (headers,
    error, detail) per block; a deferred block is ([], E_DEFERRED, 0)"""
    static = static_table()
    out = []
    for tab, blocks in decoders:
        lim = ring if tab.cap is None else min(ring, tab.cap)
        results = []
        applied = None
        for k, w in enumerate(blocks):
            fields, strings = bc.ref_scan(w)
            too_big = tab.max_size > 32 * lim or len(tab.entries) > lim  # (the ring could not hold the table)
            if applied is None and (too_big or any(f.kind == bc.SIZE_UPDATE and f.index > 32 * lim for f in fields)):
                applied = k
            if applied is not None:
                results.append(([], E_DEFERRED, 0))
                continue
            results.append(ref_apply_block(tab, fields, decode_strings(w, strings), static))
        out.append((results, len(blocks) if applied is None else applied))
    return out


# ---- block builders -------------------------------------------------------------------------------------------
def integer(value, prefix, lead):
    return hpack_ref.encode_integer(value, prefix, lead)


def raw(s):
    return integer(len(s), 7, 0) + bytes(s)


def indexed(i):
    return integer(i, 7, 0x80)


def lit_incr(name, value):
    """name: an index, or the name's bytes"""
    return (integer(name, 6, 0x40) if isinstance(name, int) else b"\x40" + raw(name)) + raw(value)


def lit_plain(name, value):
    return (integer(name, 4, 0x00) if isinstance(name, int) else b"\x00" + raw(name)) + raw(value)


def size_update(n):
    return integer(n, 5, 0x20)


def entry(k, size=40):
    """a table entry of exactly `size` octets (RFC 7541 section 4.1), its bytes naming k"""
    name = b"n%d" % k
    return name, (b"v%d-" % k).ljust(size - 32 - len(name), b".")


def long_block(nfields):
    """nfields fields: an insertion, then alternately the newest entry and a static one"""
    return lit_incr(b"x-first", b"1") + b"".join(indexed(62 if i % 2 else 2 + i % 50) for i in range(nfields - 1))


def placed(ring=2048, chunk=64):
    """[(name, Table, [block], expect)]: one decoder each. expect: per block (n_headers, error, detail) written by
    hand from RFC 7541 and decoder.rs, with optional "count" / "size" / "max_size" / "applied" of the end state.
    The cases lie relative to the kernel's geometry: its ring's records and the records a wave stages at a time."""
    out = []

    def add(name, tab, blocks, results, **end):
        out.append((name, tab, [bytes(b) for b in blocks], dict(results=results, **end)))

    C = chunk
    for n in (C - 1, C, C + 1, 2 * C, 2 * C + 1):
        add(f"a block of {n} fields", Table(), [long_block(n)], [(n, 0, 0)], count=1)
    # the chunk's edges
    fill = indexed(2) * (C - 1)
    add("an insertion in a chunk's last record, looked up by the next chunk's first", Table(),
        [fill + lit_incr(b"edge", b"v") + indexed(62)], [(C + 1, 0, 0)], count=1)
    add("an error in a chunk's first record", Table(), [indexed(2) * C + indexed(62) + indexed(2)], [(C, E_OOB, 0)])
    add("an error in a chunk's last record", Table(), [fill + indexed(62) + indexed(2)], [(C - 1, E_OOB, 0)])
    add("an error in a block's first record", Table(), [indexed(0) + indexed(2)], [(0, E_OOB, 0)])
    three = [entry(k) for k in range(3)]
    add("index 61 + count: the oldest entry", Table(three), [indexed(61 + 3)], [(1, 0, 0)], count=3)
    add("index 62 + count: out of bounds", Table(three), [indexed(62 + 3)], [(0, E_OOB, 0)], count=3)
    add("an entry inserted earlier in the same chunk", Table(), [lit_incr(b"a", b"1") + lit_incr(b"b", b"2") + indexed(63) + indexed(62)],
        [(4, 0, 0)], count=2)
    # a table that holds exactly one 40-octet entry: the insertion evicts the entry its name comes from
    add("a name taken from the entry its own insertion evicts", Table([entry(0)], max_size=40),
        [lit_incr(62, entry(0)[1]) + indexed(62)], [(2, 0, 0)], count=1, size=40)
    add("an entry of exactly max_size", Table([entry(0)], max_size=40), [lit_incr(*entry(1)) + indexed(62)], [(2, 0, 0)], count=1,
        size=40)
    add("an entry one octet above max_size empties the table", Table([entry(0)], max_size=40),
        [lit_incr(*entry(1, 41)) + indexed(62)], [(1, E_OOB, 0)], count=0, size=0)
    add("a size update to 0, then index 62", Table(three), [size_update(0) + indexed(62)], [(0, E_OOB, 0)], count=0, size=0,
        max_size=0)
    add("a shrinking size update mid-block", Table(three), [indexed(64) + size_update(80) + indexed(63) + indexed(64)],
        [(2, E_OOB, 0)], count=2, size=80, max_size=80)
    add("max_allowed exceeded", Table(three, max_allowed=100), [indexed(62) + size_update(101) + indexed(62)],
        [(1, E_INVALID_MAX, 0)], count=3, max_size=4096)
    add("max_allowed met", Table(three, max_allowed=100), [size_update(100) + indexed(63)], [(1, 0, 0)], count=2, max_size=100)
    add("a size update as the last field", Table(three), [indexed(62) + size_update(4096)], [(1, E_SU_AT_END, 0)], count=3)
    # the precedences test_gpu_blocks_device.py names
    add("a Huffman error in a name beats the value's framing error", Table(), [b"\x40" + bc.BAD_HUFF_NAME + b"\x05ab"],
        [(0, E_HUFFMAN, 2)])
    add("an indexed name out of bounds beats the value's errors", Table(), [b"\x7f\x00\x05ab"], [(0, E_OOB, 0)])
    add("SizeUpdateAtEnd comes last", Table(), [b"\x82\x20"], [(1, E_SU_AT_END, 0)], max_size=0)
    add("a Huffman error in a value, after the name's lookup", Table(), [indexed(2) + b"\x41" + bc.BAD_HUFF_NAME], [(1, E_HUFFMAN, 2)])
    add("a scan error at the index stage", Table(), [indexed(2) + b"\xff\x80"], [(1, 4, 0)])
    # more insertions than the ring has records: the ring's head wraps, 64 entries of 64 octets live
    per = 16
    nblk = (ring + 2 * C) // per + 1
    wrap = [b"".join(lit_incr(*entry(b * per + i, 64)) for i in range(per)) + indexed(62) + indexed(61 + 64) for b in range(nblk)]
    add("more insertions than the ring's records", Table(), wrap, [(per + 2, 0, 0) if b >= 3 else (per + 1, E_OOB, 0)
                                                                   for b in range(nblk)], count=64, size=4096)
    add("a decoder with no blocks", Table(three), [], [], count=3, applied=0)
    add("blocks with no fields", Table(three), [b"", indexed(62), b""], [(0, 0, 0), (1, 0, 0), (0, 0, 0)], count=3, applied=3)
    # deferral
    big = 32 * ring
    add("max_size above 32 * lim at the start", Table(three, max_size=big + 1), [indexed(62), indexed(2)],
        [(0, E_DEFERRED, 0)] * 2, count=3, max_size=big + 1, applied=0)
    add("max_size of exactly 32 * lim", Table(three, max_size=big), [indexed(62)], [(1, 0, 0)], count=3, applied=1)
    add("a size update above 32 * lim in the third block", Table(),
        [lit_incr(b"a", b"1"), lit_incr(b"b", b"2"), indexed(62) + size_update(big + 1) + indexed(2), indexed(62)],
        [(1, 0, 0), (1, 0, 0), (0, E_DEFERRED, 0), (0, E_DEFERRED, 0)], count=2, max_size=4096, applied=2)
    add("a size update of exactly 32 * lim", Table(), [size_update(big) + indexed(2)], [(1, 0, 0)], max_size=big, applied=1)
    add("a deferring size update behind the block's error", Table(), [indexed(62) + size_update(big + 1) + indexed(2)],
        [(0, E_DEFERRED, 0)], applied=0)
    add("cap below the ring's records: max_size above 32 * cap", Table(three, cap=8), [indexed(62)], [(0, E_DEFERRED, 0)], count=3,
        applied=0)
    add("cap below the ring's records: a size update above 32 * cap", Table(three, max_size=256, cap=8),
        [indexed(62), size_update(257) + indexed(2)], [(1, 0, 0), (0, E_DEFERRED, 0)], count=3, max_size=256, applied=1)
    add("cap below the ring's records: within 32 * cap", Table(three, max_size=256, cap=8), [size_update(256) + lit_incr(*entry(9))],
        [(1, 0, 0)], count=4, applied=1)
    return out


def check_expect(name, tab, results, applied, expect):
    """the placed case's edge, on any result in ref_apply's form and the table after it"""
    got = [(len(h), e, d) for h, e, d in results]
    assert got == expect["results"], (name, got[:8], expect["results"][:8])
    if "count" in expect:
        assert len(tab.entries) == expect["count"], name
    for key in ("size", "max_size"):
        if key in expect:
            assert getattr(tab, key) == expect[key], (name, key, getattr(tab, key))
    if "applied" in expect:
        assert applied == expect["applied"], name
    assert tab.size == sum(len(n) + len(v) + 32 for n, v in tab.entries), name


def rfc_truncations():
    """[(max_table_size, [the sequence's earlier blocks], truncated block)]: every proper prefix of every RFC 7541
    App. C block, with what primes its table"""
    from hpk_util import load

    out = []
    for seq in load("rfc7541_blocks.json")["sequences"]:
        for k, b in enumerate(seq["blocks"]):
            w = bytes.fromhex(b["wire"])
            before = [bytes.fromhex(p["wire"]) for p in seq["blocks"][:k]]
            out += [(seq["max_table_size"], before, w[:cut]) for cut in range(len(w))]
    return out


def primed_table(max_table_size, before, cap=None):
    """the table after `before`, by the model itself (test_blocks_apply_cases.py pins it to the oracle)"""
    tab = Table(max_size=4096 if max_table_size is None else max_table_size, cap=cap)
    ref_apply([(tab, before)], 1 << 20)
    return tab


_corpora = {}


def corpora(ring=2048, chunk=64):
    """{name: [(Table, [block])]}: the decoders every check of the apply runs over (built once; copy a Table before
    applying to it): the interop stories, the seeded corruptions the scan's tests use, the random and the scan's
    placed blocks one decoder each, every truncation of the RFC 7541 App. C blocks on its primed table, and the
    apply's own placed cases"""
    key = (ring, chunk)
    if key not in _corpora:
        c = {}
        c["interop"] = [(Table(), [bytes.fromhex(x["wire"]) for x in story["cases"]]) for _, story in bc.stories()]
        c["corrupted"] = [(Table(), blocks) for blocks in bc.corrupted_stories()]
        c["corrupted9"] = [(Table(), blocks) for blocks in bc.corrupted_stories(seed=9, nstories=12)]
        c["random"] = [(Table(), [w]) for w in bc.random_blocks() + [b for _, b, _ in bc.placed()]]
        c["rfc"] = [(primed_table(size, before), [w]) for size, before, w in rfc_truncations()]
        c["placed"] = [(tab, blocks) for _, tab, blocks, _ in placed(ring, chunk)]
        _corpora[key] = c
    return _corpora[key]


def fresh(decoders):
    return [(tab.copy(), blocks) for tab, blocks in decoders]
