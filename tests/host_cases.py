"""Case files of the stand-alone host driver (tests/host/host_driver.cpp has the format): the inputs from the
generators the suite's other tests use, the expected results from oracle/hpack_ref.py and the C oracle alone.

A section writer returns (bytes, cases): the section's body and the number of cases the driver counts in it (a block,
a table at the end, a connection of a call, a literal), so the test can assert the `ok:` line's count.
tests/test_host_sanitizers.py puts the sections together."""

import random
import struct

import blocks_apply_cases as ac
import blocks_scan_cases as bc
import h2_cases as hc
from hpack_cases import churn_streams
from hpk_util import hpack_ref, load, oracle_decode, oracle_encode

MAGIC = 0x434B5048
DECODE, ENCODE, H2, HUFFMAN, THREADS, FORK = 1, 2, 3, 4, 5, 6

# hpk_block_error of a hpack_ref.DecoderError (include/hpk.h)
_INT = {"TooManyOctets": 2, "ValueTooLarge": 3, "NotEnoughOctets": 4, "InvalidPrefix": 5}


def u32(*xs):
    return struct.pack("<%dI" % len(xs), *(x & 0xFFFFFFFF for x in xs))


def blob(b):
    return u32(len(b)) + bytes(b)


def error_code(e):
    """(hpk_block_error, detail) of a hpack_ref.DecoderError, (0, 0) for None"""
    if e is None:
        return 0, 0
    if e.kind == "HeaderIndexOutOfBounds":
        return 1, 0
    if e.kind == "IntegerDecodingError":
        return _INT[e.detail], 0
    if e.kind == "StringDecodingError":
        return (6, 0) if e.detail == "NotEnoughOctets" else (7, e.detail[1])
    return {"InvalidMaxDynamicSize": 8, "SizeUpdateAtEnd": 9}[e.kind], 0


def headers(hs):
    return b"".join(blob(n) + blob(v) for n, v in hs)


# ---- decode --------------------------------------------------------------------------------------------------------
class Dec:
    """one decoder of a decode section: how the driver sets it up, and the reference decoder in the same state"""

    def __init__(self, tab=None):
        self.ref = hpack_ref.Decoder()
        self.max_size = self.max_allowed = None
        self.prime = []
        if tab is not None:  # a blocks_apply_cases.Table: its entries go in through one block of insertions, oldest first
            if tab.max_size != 4096:
                self.max_size = tab.max_size
            if tab.entries:
                self.prime = [b"".join(ac.lit_incr(n, v) for n, v in reversed(tab.entries))]
            self.max_allowed = tab.max_allowed
            self.ref.dynamic.table = list(tab.entries)
            self.ref.dynamic.size = tab.size
            self.ref.dynamic.max_size = tab.max_size
            self.ref.max_allowed_table_size = tab.max_allowed


def decode_section(decs, calls):
    """decs: [Dec]; calls: [[(index of its Dec, block)]], each call's blocks in order -> (body, cases)"""
    out = [u32(len(decs))]
    for d in decs:
        out.append(u32(d.max_size is not None, d.max_size or 0, d.max_allowed is not None, d.max_allowed or 0, len(d.prime)))
        out += [blob(w) for w in d.prime]
    out.append(u32(len(calls)))
    cases = 0
    for call in calls:
        out.append(u32(len(call)))
        for k, w in call:
            hs, err = hc.decode_with_error(decs[k].ref, w)
            out.append(u32(k) + blob(w) + u32(len(hs), *error_code(err)) + headers(hs))
            cases += 1
    for d in decs:
        out.append(u32(d.ref.dynamic.size, len(d.ref.dynamic.table), d.ref.dynamic.max_size))
        cases += 1
    return b"".join(out), cases


def from_decoders(decoders):
    """[(Table, [block])] (blocks_apply_cases' form), every block of every decoder in ONE call, decoder after decoder"""
    decs = [Dec(tab) for tab, _ in decoders]
    return decs, [[(k, w) for k, (_, blocks) in enumerate(decoders) for w in blocks]]


def interop_slice(min_blocks=1024, start=0):
    """whole interop stories, one decoder each, from story `start` on until they hold at least min_blocks blocks"""
    out, n = [], 0
    for _, story in list(bc.stories())[start:]:
        blocks = [bytes.fromhex(c["wire"]) for c in story["cases"]]
        out.append((ac.Table(), blocks))
        n += len(blocks)
        if n >= min_blocks:
            break
    assert n >= min_blocks
    return out


def decode_corpora():
    """{name: [(Table, [block])]}: blocks_apply_cases.corpora() (the seeded corruptions, the random and the scan's placed
    blocks, every truncation of the RFC 7541 App. C blocks on its primed table, the apply's placed cases: table-size
    updates, eviction, deferral edges) with a slice of the interop stories in place of all of them, every proper
    prefix of the RFC blocks on a fresh decoder, the churn streams, and the Huffman error vectors inside blocks"""
    c = {k: ac.fresh(v) for k, v in ac.corpora().items() if k != "interop"}
    c["interop"] = interop_slice(2048)
    c["rfc_prefixes"] = [(ac.Table(), [w]) for w in bc.rfc_prefixes()]
    c["churn"] = [(ac.Table(), blocks) for blocks in churn_streams()]
    c["huffman"] = [(ac.Table(), [w]) for w in huffman_error_blocks()]
    return c


def huffman_error_blocks(step=8):
    """the reference's Huffman error vectors (every step-th: PaddingTooLarge, InvalidPadding, EOSInString) as the value
    string of one block and as the name string of another, behind a header that is emitted first"""
    out = []
    for v in [x for x in load("error_vectors.json")["vectors"] if x["status"] != 0][::step]:
        s = bytes.fromhex(v["in"])
        h = ac.integer(len(s), 7, 0x80) + s
        out.append(ac.indexed(2) + b"\x40" + ac.raw(b"x-name") + h)
        out.append(ac.indexed(2) + b"\x00" + h + ac.raw(b"value"))
    return out


# ---- encode --------------------------------------------------------------------------------------------------------
SINGLE, BLOCKS, SINGLE_NOSPACE, BLOCKS_FAILED = 0, 1, 2, 3


def encode_section(specs, calls):
    """specs: [(huffman, max_size or None)]; calls: [(kind, [(encoder index, [(name, value)])])] -> (body, cases)"""
    refs = []
    out = [u32(len(specs))]
    for huffman, max_size in specs:
        r = hpack_ref.Encoder(huffman=bool(huffman))
        if max_size is not None:
            r.set_max_table_size(max_size)
        refs.append(r)
        out.append(u32(bool(huffman), max_size is not None, max_size or 0))
    out.append(u32(len(calls)))
    cases = 0
    for kind, blocks in calls:
        assert kind in (BLOCKS, BLOCKS_FAILED) or len(blocks) == 1
        out.append(u32(kind, len(blocks)))
        for k, hs in blocks:
            out.append(u32(k, len(hs)) + headers(hs) + blob(refs[k].encode(hs)))
        cases += 1 if kind in (SINGLE, SINGLE_NOSPACE) else len(blocks)
    for r in refs:
        out.append(u32(r.dynamic.size, len(r.dynamic.table), r.dynamic.max_size))
        cases += 1
    return b"".join(out), cases


def story_lists(step=1):
    inter = load("interop.json.gz")
    return [[[(n.encode(), v.encode()) for n, v in c["headers"]] for c in story["cases"]]
            for enc in sorted(inter) for story in inter[enc]][::step]


def encode_single_calls(stories):
    """every header list of `stories` through hpk_henc_encode, one encoder per story (Huffman on for every other one, a
    small table for every third), every fifth call first with cap one below the need"""
    specs = [(k % 2, (None, 256, 100)[k % 3]) for k in range(len(stories))]
    calls = []
    for k, lists in enumerate(stories):
        for hs in lists:
            calls.append((SINGLE_NOSPACE if len(calls) % 5 == 0 else SINGLE, [(k, hs)]))
    return specs, calls


def encode_block_calls(stories, per_call=40, seed=3):
    """the header lists of `stories` through hpk_henc_encode_blocks, per_call stories a call with their blocks
    interleaved (each encoder's in order), seeded random lists (text, binary, empty) on two more encoders, and one call
    of Huffman-coding encoders first with an injected batch failure"""
    rng = random.Random(seed)
    specs = [(k % 2, (None, 256)[k % 2 ^ k // 2 % 2]) for k in range(len(stories))] + [(1, None), (0, 100)]
    calls = []
    for lo in range(0, len(stories), per_call):
        group = list(range(lo, min(lo + per_call, len(stories))))
        depth = max(len(stories[k]) for k in group)
        blocks = [(k, stories[k][i]) for i in range(depth) for k in group if i < len(stories[k])]
        calls.append((BLOCKS_FAILED if lo == per_call else BLOCKS, blocks))
    blocks = []
    for i in range(200):
        hs = []
        for _ in range(rng.randrange(0, 8)):
            k = rng.choice([b"content-type", b"x-req-id", b"set-cookie", b"server", b":status", b""])
            v = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 40))) if rng.random() < 0.3 else \
                str(rng.randrange(10**9)).encode()
            hs.append((k, v))
        blocks.append((len(stories) + i % 2, hs))
    calls.append((BLOCKS, blocks))
    calls.append((BLOCKS, []))  # an empty call
    return specs, calls


# ---- h2 ------------------------------------------------------------------------------------------------------------
class H2Section:
    """connections and calls as they are added; ref_read (h2_cases) gives what each call must return"""

    def __init__(self):
        self.conns, self.frame_sizes, self.calls, self.cases = [], [], [], 0
        self.seen_errors = set()

    def conn(self, max_frame_size=None):
        self.conns.append(hc.RefConn(max_frame_size or 16384))
        self.frame_sizes.append(max_frame_size or 0)
        return len(self.conns) - 1

    def call(self, ids, chunks):
        """-> (errors, consumed, blocks) of the call by the model"""
        errors, consumed, blocks = hc.ref_read([self.conns[k] for k in ids], chunks)
        out = [u32(len(ids))]
        for k, data, e, n in zip(ids, chunks, errors, consumed):
            out.append(u32(k) + blob(data) + u32(e, n))
        out.append(u32(len(blocks)))
        for c, sid, es, skipped, hs, err in blocks:
            out.append(u32(c, sid, es, skipped, len(hs), *error_code(err)) + headers(hs))
        self.calls.append(b"".join(out))
        self.cases += len(ids) + len(blocks)
        self.seen_errors |= set(errors)
        return errors, consumed, blocks

    def body(self):
        out = u32(len(self.conns), *self.frame_sizes) + u32(len(self.calls)) + b"".join(self.calls)
        return out + u32(*[c.error for c in self.conns]), self.cases + len(self.conns)


def h2_replay(sec, wires, calls=4, seed=1):
    """every connection's bytes in `calls` random cuts, an incomplete frame sent again with the next bytes (tests/test_h2.py's
    replay) -> the blocks per connection"""
    rng = random.Random(seed)
    ids = [sec.conn() for _ in wires]
    cuts = [sorted(rng.sample(range(len(w) + 1), calls - 1)) + [len(w)] for w in wires]
    pos = [0] * len(wires)
    got = [[] for _ in wires]
    for k in range(calls):
        errors, consumed, blocks = sec.call(ids, [wires[c][pos[c] : cuts[c][k]] for c in range(len(wires))])
        assert errors == [hc.H2_OK] * len(wires)
        pos = [p + n for p, n in zip(pos, consumed)]
        for c, sid, es, skipped, hs, err in blocks:
            assert not skipped and err is None
            got[c].append((sid, bool(es), hs))
    assert pos == [len(w) for w in wires]
    return got


def h2_section(step=4):
    """the frame sequences of tests/test_h2.py: every step-th interop connection replayed in four random cuts and in a
    single call, the placed error sequences, the httpwg cases, a compression error that stops its connection, an
    incomplete frame and a pending CONTINUATION carried across calls, and set_max_frame_size at its edges. The
    model is pinned here to the expectations tests/test_h2.py states by hand."""
    sec = H2Section()
    wires, wants = hc.interop_connections(0)
    assert h2_replay(sec, wires[::step]) == [[(s, e, h) for s, e, h in w] for w in wants[::step]]
    wires, wants = hc.interop_connections(7)
    ids = [sec.conn() for _ in wires[::step]]
    errors, consumed, blocks = sec.call(ids, wires[::step])
    assert errors == [0] * len(ids) and consumed == [len(w) for w in wires[::step]]
    got = [[] for _ in ids]
    for c, sid, es, skipped, hs, err in blocks:
        got[c].append((sid, bool(es), hs))
    assert got == wants[::step]

    def one(frames, want_err, want_blocks=None):
        k = sec.conn()
        errors, _, blocks = sec.call([k], [b"".join(frames)])
        assert errors == [hc.H2_NAMES[want_err]], (errors, want_err)
        if want_blocks is not None:
            assert [(sid, es, hs) for _, sid, es, _, hs, _ in blocks] == want_blocks
        return k, blocks

    F, B = hc.frame, hc.BLOCK
    for second, err in hc.CHECK_ORDER:
        one([F(hc.HEADERS, 0, 1, B[:5]), second], err, [])
    for frames, err, _ in hc.CONNECTION_ERRORS:
        one(frames, err)
    _, blocks = one([F(hc.HEADERS, hc.END_STREAM | hc.END_HEADERS, 1, b"\x40")], "HpackDecodingError")
    assert blocks[0][5].kind == "IntegerDecodingError"
    one([F(hc.HEADERS, hc.END_HEADERS, 1, B), F(hc.PRIORITY, 0, 1, b"\0\0\0\0\xff"), F(hc.CONTINUATION, hc.END_HEADERS, 1, B)],
        "UnexpectedContinuationFrame", [(1, 0, hc.C41)])
    one([F(hc.HEADERS, 0, 1, B), F(hc.HEADERS, hc.END_HEADERS, 3, B)], "ExpectedContinuationForStream", [])
    one([F(hc.HEADERS, hc.PADDED | hc.PRIO | hc.END_STREAM, 5, bytes([4]) + b"\0\0\0\x07\x20" + B[:3] + b"\0" * 4),
         F(hc.CONTINUATION, 0, 5, B[3:9]), F(hc.CONTINUATION, hc.END_HEADERS, 5, B[9:])], None, [(5, 1, hc.C41)])
    # a compression error stops its connection: the later block of the call skipped, the connection dead afterwards
    bad, good = F(hc.HEADERS, hc.END_HEADERS, 1, b"\x40"), F(hc.HEADERS, hc.END_HEADERS, 3, B)
    a, b = sec.conn(), sec.conn()
    errors, _, blocks = sec.call([a, b], [bad + good, good])
    assert errors == [hc.COMPRESSION_ERROR, 0] and [(x[0], x[1], x[3]) for x in blocks] == [(0, 1, 0), (0, 3, 1), (1, 3, 0)]
    errors, consumed, blocks = sec.call([a, b], [good, F(hc.HEADERS, hc.END_HEADERS, 5, bytes.fromhex("828684be"))])
    assert errors == [hc.COMPRESSION_ERROR, 0] and consumed[0] == 0 and [(x[0], x[1], x[4]) for x in blocks] == [(1, 5, hc.C41)]
    # an incomplete frame and a pending CONTINUATION carried across calls: mid-header, mid-payload, between frames, the end
    frames = F(hc.HEADERS, 0, 1, B[:4]) + F(hc.CONTINUATION, hc.END_HEADERS, 1, B[4:])
    k, pos, got = sec.conn(), 0, []
    for cut in (3, 9, 15, len(frames)):
        errors, consumed, blocks = sec.call([k], [frames[pos:cut]])
        assert errors == [0]
        pos += consumed[0]
        got += [(x[1], x[2], x[4]) for x in blocks]
    assert pos == len(frames) and got == [(1, 0, hc.C41)]
    # set_max_frame_size: a frame of exactly the limit passes, one octet more is FrameTooLarge; the default's edge too
    big = sec.conn(20000)
    errors, consumed, _ = sec.call([big], [F(hc.DATA, 0, 1, b"x" * 20000) + F(hc.HEADERS, hc.END_HEADERS, 3, B)])
    assert errors == [0] and consumed == [2 * 9 + 20000 + len(B)]
    errors, consumed, _ = sec.call([big], [F(hc.DATA, 0, 1, b"x" * 20001)])
    assert errors == [hc.FRAME_TOO_LARGE] and consumed == [0]
    k = sec.conn()
    errors, _, _ = sec.call([k], [F(hc.DATA, 0, 1, b"x" * 16384)])
    assert errors == [0]
    # a frame header announcing more than the limit is refused before its payload has arrived
    errors, consumed, _ = sec.call([sec.conn()], [F(hc.DATA, 0, 1, b"x" * 16385)[:9]])
    assert errors == [hc.FRAME_TOO_LARGE] and consumed == [0]
    sec.call([], [])  # a call with no connection
    return sec


# ---- huffman -------------------------------------------------------------------------------------------------------
def huffman_section(nrandom=300, seed=5):
    """literals for the single-literal entry points and the CPU batch calls: the reference's known answers and error
    vectors, a sample of the interop corpus' literals and seeded random bytes (decode); text, binary and empty strings
    (encode). Expected results by the C oracle, the decode also at one byte below the decoded length."""
    import ctypes

    from hpk_util import interop_literals, oracle

    rng = random.Random(seed)
    lits = [bytes.fromhex(k["in"]) for k in load("kat.json")]
    lits += [bytes.fromhex(v["in"]) for v in load("error_vectors.json")["vectors"]][::4]
    lits += interop_literals()[::40]
    lits += [bytes(rng.getrandbits(8) for _ in range(rng.randrange(0, 40))) for _ in range(nrandom)]
    lits.append(b"")
    out = [u32(len(lits))]
    statuses = set()
    for w in lits:
        st, dec = oracle_decode(w)
        st1, dec1 = 0, b""
        if dec:  # the oracle at one byte below the decoded length
            L = oracle()
            buf = ctypes.create_string_buffer(len(dec))
            ol = ctypes.c_size_t(0)
            st1 = L.oracle_decode(bytes(w), len(w), buf, len(dec) - 1, ctypes.byref(ol))
            dec1 = buf.raw[: ol.value]
        statuses.add(st)
        out.append(blob(w) + u32(st) + blob(dec) + u32(st1) + blob(dec1))
    plain = [bytes(rng.getrandbits(8) for _ in range(rng.randrange(0, 60))) for _ in range(nrandom)]
    plain += [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz0123456789-/ ") for _ in range(rng.randrange(0, 200))) for _ in range(nrandom)]
    plain += [b"", bytes(range(256))]
    out.append(u32(len(plain)))
    for s in plain:
        out.append(blob(s) + blob(oracle_encode(s)))
    return b"".join(out), len(lits) + len(plain), statuses


def case_file(sections):
    """[(tag, body)] -> the file's bytes"""
    return u32(MAGIC) + b"".join(u32(tag) + body for tag, body in sections) + u32(0)
