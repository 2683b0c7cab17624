"""The header-block scan's reference tokeniser and its placed cases (hpk_scan_blocks, loona_amd/csrc/hpk_blkscan.h).

ref_scan(block) is the table-free half of Decoder::decode_with_cb (decoder.rs:368-450) restated on
hpack_ref.decode_integer alone: per field the kind, decode_integer's value, the exact windows of the strings whose
prefix and length check passed, and an integer or length error with the stage at which the reference would raise it.
tests/test_blocks_scan_cases.py pins it to hpack_ref.Decoder by applying its tokens; the emulation and the GPU tests
compare the kernels' walk with it."""

import random
from collections import namedtuple

from hpk_util import hpack_ref, load

# hpk_field_kind
INDEXED, LIT_INCR, SIZE_UPDATE, LIT_NEVER, LIT_PLAIN = range(5)
# hpk_block_error values the scan can find
E_OK, E_INT_TOO_MANY, E_INT_SHORT, E_STR_SHORT = 0, 2, 4, 6
ST_INDEX, ST_NAME, ST_VALUE = 0, 1, 2

Field = namedtuple("Field", "index str kind nstr err err_stage at")  # hpk_field, offsets relative to the block

_INT_ERR = {"TooManyOctets": E_INT_TOO_MANY, "NotEnoughOctets": E_INT_SHORT}


def _kind(b):
    if b & 128:
        return INDEXED, 7
    if b & 64:
        return LIT_INCR, 6
    if b & 32:
        return SIZE_UPDATE, 5
    return (LIT_NEVER, 4) if b & 16 else (LIT_PLAIN, 4)


def ref_scan(block):
    """-> (fields, strings): [Field], [(off, end)] with block-relative offsets and string indices"""
    block = bytes(block)
    fields, strings = [], []
    pos = 0
    while pos < len(block):
        kind, prefix = _kind(block[pos])
        first = len(strings)
        try:
            index, used = hpack_ref.decode_integer(block[pos:], prefix)
        except hpack_ref.DecoderError as e:
            fields.append(Field(0, first, kind, 0, _INT_ERR[e.detail], ST_INDEX, pos))
            break
        at = pos + used
        err, stage, nstr = E_OK, ST_INDEX, 0
        if kind in (LIT_INCR, LIT_NEVER, LIT_PLAIN):
            for st in ((ST_NAME, ST_VALUE) if index == 0 else (ST_VALUE,)):
                try:
                    ln, c = hpack_ref.decode_integer(block[at:], 7)
                except hpack_ref.DecoderError as e:
                    err, stage = _INT_ERR[e.detail], st
                    break
                if c + ln > len(block) - at:
                    err, stage = E_STR_SHORT, st
                    break
                strings.append((at, at + c + ln))
                nstr += 1
                at += c + ln
        fields.append(Field(index, first, kind, nstr, err, stage, pos))
        if err:
            break
        pos = at
    return fields, strings


LEAD = {INDEXED: (0x80, 127), LIT_INCR: (0x40, 63), SIZE_UPDATE: (0x20, 31), LIT_NEVER: (0x10, 15), LIT_PLAIN: (0x00, 15)}
_IS_LIT = {LIT_INCR, LIT_NEVER, LIT_PLAIN}

# a name whose Huffman payload is wrong: '0' (00000) then padding 000: InvalidPadding
BAD_HUFF_NAME = bytes([0x81, 0x00])


def placed():
    """[(name, block, expect)]: expect holds what the case's edge means for the scan, written from RFC 7541 and
    decoder.rs by hand (not from ref_scan): nfields, nstrs, and the last field's index / nstr / err / err_stage."""
    out = []

    def add(name, block, **expect):
        out.append((name, bytes(block), expect))

    val = b"\x01a"  # a value string
    for kind, (lead, mask) in LEAD.items():
        tail = val if kind in _IS_LIT else b""
        ns = 1 if kind in _IS_LIT else 0
        add(f"kind {kind}: 1-octet integer", bytes([lead | 1]) + tail, nfields=1, nstrs=ns, index=1, err=0, kind=kind)
        add(f"kind {kind}: 2-octet integer", bytes([lead | mask, 5]) + tail, nfields=1, nstrs=ns, index=mask + 5, err=0,
            kind=kind)
        add(f"kind {kind}: 5-octet integer", bytes([lead | mask, 0x80, 0x80, 0x80, 0x01]) + tail, nfields=1, nstrs=ns,
            index=mask + (1 << 21), err=0, kind=kind)
        add(f"kind {kind}: largest 5-octet integer", bytes([lead | mask, 0xFF, 0xFF, 0xFF, 0x7F]) + tail, nfields=1,
            nstrs=ns, index=mask + (1 << 28) - 1, err=0, kind=kind)
        add(f"kind {kind}: 5th octet continues", bytes([0x82, lead | mask, 0x80, 0x80, 0x80, 0x80]), nfields=2, nstrs=0,
            err=E_INT_TOO_MANY, err_stage=ST_INDEX, kind=kind)
        add(f"kind {kind}: 5th octet continues, more follows", bytes([lead | mask, 0xFF, 0xFF, 0xFF, 0xFF, 0x00, 0x82]),
            nfields=1, nstrs=0, err=E_INT_TOO_MANY, err_stage=ST_INDEX, kind=kind)
        for cut in (2, 3, 4):
            add(f"kind {kind}: integer cut after {cut} octets", bytes([lead | mask] + [0x80] * (cut - 1)), nfields=1, nstrs=0,
                err=E_INT_SHORT, err_stage=ST_INDEX, kind=kind)
        # the all-ones first octet at the block's end, and one octet before it
        allones = lead | mask
        add(f"0x{allones:02x} at the block's end", bytes([0x82, allones]), nfields=2, nstrs=0, err=E_INT_SHORT,
            err_stage=ST_INDEX, kind=kind)
        if kind in _IS_LIT:  # the integer ends with the block: the value string's prefix is missing
            add(f"0x{allones:02x} one octet before the block's end", bytes([0x82, allones, 0x00]), nfields=2, nstrs=0,
                index=mask, err=E_INT_SHORT, err_stage=ST_VALUE, kind=kind)
        else:
            add(f"0x{allones:02x} one octet before the block's end", bytes([0x82, allones, 0x00]), nfields=2, nstrs=0,
                index=mask, err=0, kind=kind)
    # strings against the block's end
    add("string ends exactly at the block's end", b"\x01\x03abc", nfields=1, nstrs=1, nstr=1, err=0, windows=[(1, 5)])
    add("string ends one octet past the block's end", b"\x01\x04abc", nfields=1, nstrs=0, nstr=0, err=E_STR_SHORT,
        err_stage=ST_VALUE)
    add("name ends one octet past the block's end", b"\x00\x04abc", nfields=1, nstrs=0, nstr=0, err=E_STR_SHORT,
        err_stage=ST_NAME)
    add("empty raw string", b"\x01\x00", nfields=1, nstrs=1, nstr=1, err=0, windows=[(1, 2)])
    add("empty Huffman string", b"\x41\x80", nfields=1, nstrs=1, nstr=1, err=0, windows=[(1, 2)])
    add("empty name and empty value", b"\x10\x00\x00", nfields=1, nstrs=2, nstr=2, err=0, windows=[(1, 2), (2, 3)])
    add("string length 127 + 2^28 - 1 in a short block", b"\x01\x7f\xff\xff\xff\x7f", nfields=1, nstrs=0, err=E_STR_SHORT,
        err_stage=ST_VALUE)
    add("string length prefix: 5th octet continues (name)", b"\x00\x7f\x80\x80\x80\x80\x00", nfields=1, nstrs=0,
        err=E_INT_TOO_MANY, err_stage=ST_NAME)
    add("string length prefix: 5th octet continues (value)", b"\x01\xff\x80\x80\x80\x80", nfields=1, nstrs=0,
        err=E_INT_TOO_MANY, err_stage=ST_VALUE)
    add("string length prefix cut (value)", b"\x01\x7f\x80", nfields=1, nstrs=0, err=E_INT_SHORT, err_stage=ST_VALUE)
    add("a 2-octet string length", b"\x01\x7f\x01" + b"x" * 128, nfields=1, nstrs=1, nstr=1, err=0, windows=[(1, 131)])
    # name index 0 against nonzero
    add("name index 0: two strings", b"\x00\x01a\x01b", nfields=1, nstrs=2, nstr=2, index=0, err=0, windows=[(1, 3), (3, 5)])
    add("name index 2: one string", b"\x02\x01b", nfields=1, nstrs=1, nstr=1, index=2, err=0, windows=[(1, 3)])
    add("name index 0 with nothing after it", b"\x82\x40", nfields=2, nstrs=0, nstr=0, err=E_INT_SHORT, err_stage=ST_NAME)
    add("name listed, value missing", b"\x40\x01a", nfields=1, nstrs=1, nstr=1, err=E_INT_SHORT, err_stage=ST_VALUE,
        windows=[(1, 3)])
    # a Huffman error in the name (found only by the string decode) before a value that is cut short
    add("bad Huffman name, value cut short", b"\x40" + BAD_HUFF_NAME + b"\x05ab", nfields=1, nstrs=1, nstr=1, err=E_STR_SHORT,
        err_stage=ST_VALUE, windows=[(1, 3)])
    add("bad Huffman name, good value", b"\x40" + BAD_HUFF_NAME + b"\x02ab", nfields=1, nstrs=2, nstr=2, err=0)
    # a size update as the last field (SizeUpdateAtEnd is the apply's to find)
    add("size update last", b"\x82\x20", nfields=2, nstrs=0, err=0, kind=SIZE_UPDATE, index=0)
    add("size update then a field", b"\x3f\xe1\x1f\x82", nfields=2, nstrs=0, err=0, kind=INDEXED, index=2)
    add("empty block", b"", nfields=0, nstrs=0)
    for b in range(256):
        kind, prefix = _kind(b)
        mask = (1 << prefix) - 1
        if b & mask == mask:
            exp = dict(err=E_INT_SHORT, err_stage=ST_INDEX)
        elif kind not in _IS_LIT:
            exp = dict(err=0, index=b & mask)
        else:
            exp = dict(err=E_INT_SHORT, err_stage=ST_NAME if b & mask == 0 else ST_VALUE, index=b & mask)
        add(f"one-octet block 0x{b:02x}", bytes([b]), nfields=1, nstrs=0, kind=kind, **exp)
    return out


def rfc_blocks():
    g = load("rfc7541_blocks.json")
    return [bytes.fromhex(b["wire"]) for seq in g["sequences"] for b in seq["blocks"]]


def rfc_prefixes():
    """every proper prefix of every RFC 7541 App. C block"""
    return [w[:cut] for w in rfc_blocks() for cut in range(len(w))]


def check_expect(name, block, fields, strings, expect):
    """the placed case's edge, on any scan result in ref_scan's form"""
    assert len(fields) == expect["nfields"], name
    assert len(strings) == expect["nstrs"], name
    if not fields:
        return
    last = fields[-1]
    for key in ("index", "nstr", "err", "err_stage", "kind"):
        if key in expect:
            assert getattr(last, key) == expect[key], (name, key, last)
    if "windows" in expect:
        assert strings == expect["windows"], name
    for f in fields[:-1]:
        assert f.err == 0, name


def stories():
    inter = load("interop.json.gz")
    for enc in sorted(inter):
        for story in inter[enc]:
            yield enc, story


def interop_blocks():
    return [bytes.fromhex(c["wire"]) for _, story in stories() for c in story["cases"]]


def mutate(rng, w):
    """test_hpack.py's corruptions: a bit flip, a truncation, an insertion, random bytes"""
    w = bytearray(w)
    op = rng.randrange(4)
    if op == 0 and w:
        w[rng.randrange(len(w))] ^= 1 << rng.randrange(8)
    elif op == 1 and w:
        del w[rng.randrange(len(w)) :]
    elif op == 2:
        w[rng.randrange(len(w) + 1) : 0] = bytes(rng.getrandbits(8) for _ in range(rng.randrange(1, 6)))
    else:
        for _ in range(rng.randrange(1, 4)):
            if w:
                w[rng.randrange(len(w))] = rng.getrandbits(8)
    return bytes(w)


def corrupted_stories(seed=7541, nstories=40, per_story=12):
    """[[block]]: seeded corruptions of interop stories, a list of blocks per story (one decoder each)"""
    rng = random.Random(seed)
    out = []
    for story in rng.sample([s for _, s in stories()], nstories):
        blocks = []
        for c in story["cases"][:per_story]:
            w = bytes.fromhex(c["wire"])
            blocks.append(mutate(rng, w) if rng.random() < 0.5 else w)
        out.append(blocks)
    return out


def random_blocks(seed=11, n=3000):
    rng = random.Random(seed)
    return [bytes(rng.getrandbits(8) for _ in range(rng.randrange(0, 24))) for _ in range(n)]


FIELD_DTYPE = [("index", "<u4"), ("str", "<u4"), ("kind", "u1"), ("nstr", "u1"), ("err", "u1"), ("err_stage", "u1"),
               ("at", "<u4")]  # hpk_field

Batch = namedtuple("Batch", "blob block_off fields field_off str_off str_end str_blk_off")


def expected_batch(blocks, base=0):
    """hpk_scan_blocks' answer for `blocks` laid end to end from offset `base` of the blob, by ref_scan: the blob
    (base zero bytes first), block_off, the hpk_field records (absolute `at` and string indices), field_off, the
    string windows and str_blk_off, as numpy arrays"""
    import numpy as np

    recs, so, se, foff, soff, boff = [], [], [], [0], [0], [base]
    for w in blocks:
        fields, strings = ref_scan(w)
        at, s0 = boff[-1], soff[-1]
        recs += [(f.index, s0 + f.str, f.kind, f.nstr, f.err, f.err_stage, at + f.at) for f in fields]
        so += [at + a for a, _ in strings]
        se += [at + e for _, e in strings]
        foff.append(foff[-1] + len(fields))
        soff.append(s0 + len(strings))
        boff.append(at + len(w))
    blob = np.frombuffer(bytes(base) + b"".join(blocks), dtype=np.uint8).copy()
    u = lambda x: np.asarray(x, dtype=np.int64).astype(np.uint32)  # noqa: E731
    return Batch(blob, u(boff), np.array(recs, dtype=FIELD_DTYPE), u(foff), u(so), u(se), u(soff))
