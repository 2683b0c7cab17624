"""blocks_scan_cases.ref_scan pinned to the oracle (no GPU, no library).

ref_scan tokenises a block with no decoder in hand. Here its tokens are applied with hpack_ref's tables and string
decode in a few lines, in the order hpk_hdec_decode_blocks' apply uses; the result must reproduce
hpack_ref.Decoder.decode (the headers, or the first error) on the interop stories, the RFC 7541 App. C sequences
and error vectors, seeded corruptions with the table carried across a story's blocks, 3,000 random short blocks,
every proper prefix of the RFC blocks and every placed case. So whatever equals ref_scan (the kernels' walk in the
emulation and on the GPU) scans as the reference does."""

import blocks_scan_cases as bc
from hpk_util import hpack_ref, load

_ERR = {bc.E_INT_TOO_MANY: ("IntegerDecodingError", "TooManyOctets"), bc.E_INT_SHORT: ("IntegerDecodingError", "NotEnoughOctets"),
        bc.E_STR_SHORT: ("StringDecodingError", "NotEnoughOctets")}


def apply_tokens(dec, block, fields, strings):
    """the reference's single pass over ref_scan's tokens: the headers, or raises the first error"""
    out = []

    def fail(f):
        raise hpack_ref.DecoderError(*_ERR[f.err])

    def string(s):
        a, e = strings[s]
        data, consumed = hpack_ref.decode_string(block[a:e])  # (raises the Huffman error)
        assert consumed == e - a
        return data

    last_update = False
    for f in fields:
        last_update = f.kind == bc.SIZE_UPDATE
        if f.err and f.err_stage == bc.ST_INDEX:
            fail(f)
        if f.kind == bc.INDEXED:
            out.append(dec.get_from_table(f.index))
        elif f.kind == bc.SIZE_UPDATE:
            if dec.max_allowed_table_size is not None and f.index > dec.max_allowed_table_size:
                raise hpack_ref.DecoderError("InvalidMaxDynamicSize")
            dec.dynamic.set_max_table_size(f.index)
        else:
            s = f.str
            if f.index == 0:
                if f.err and f.err_stage == bc.ST_NAME:
                    fail(f)
                name = string(s)
                s += 1
            else:
                name = dec.get_from_table(f.index)[0]
            if f.err and f.err_stage == bc.ST_VALUE:
                fail(f)
            value = string(s)
            out.append((name, value))
            if f.kind == bc.LIT_INCR:
                dec.dynamic.add_header(name, value)
    if last_update:
        raise hpack_ref.DecoderError("SizeUpdateAtEnd")
    return out


def _both(block, d_ref, d_tok, seen=None):
    """decode `block` by the oracle and by ref_scan + apply_tokens on twin decoders; both must agree"""
    def run(fn):
        try:
            return fn()
        except hpack_ref.DecoderError as e:
            return (e.kind, e.detail)

    fields, strings = bc.ref_scan(block)
    want = run(lambda: d_ref.decode(block))
    got = run(lambda: apply_tokens(d_tok, block, fields, strings))
    assert got == want, (block.hex(), got, want)
    assert d_ref.dynamic.table == d_tok.dynamic.table and d_ref.dynamic.max_size == d_tok.dynamic.max_size, block.hex()
    if seen is not None:
        if isinstance(want, tuple):
            seen["kinds"].add((want[0], want[1] if not isinstance(want[1], tuple) else want[1][0]))
        if fields and fields[-1].err:
            seen["stages"].add(fields[-1].err_stage)
    return want


def test_interop_stories():
    n = 0
    for _, story in bc.stories():
        d, t = hpack_ref.Decoder(), hpack_ref.Decoder()
        for c in story["cases"]:
            got = _both(bytes.fromhex(c["wire"]), d, t)
            assert got == [(a.encode(), b.encode()) for a, b in c["headers"]]
            n += 1
    assert n > 16000


def test_rfc_sequences_and_error_vectors():
    g = load("rfc7541_blocks.json")
    for seq in g["sequences"]:
        d, t = hpack_ref.Decoder(), hpack_ref.Decoder()
        if seq["max_table_size"] is not None:
            d.set_max_table_size(seq["max_table_size"])
            t.set_max_table_size(seq["max_table_size"])
        for b in seq["blocks"]:
            got = _both(bytes.fromhex(b["wire"]), d, t)
            assert [[n.decode(), v.decode()] for n, v in got] == b["headers"]
    for e in g["errors"]:
        got = _both(bytes.fromhex(e["wire"]), hpack_ref.Decoder(), hpack_ref.Decoder())
        assert isinstance(got, tuple), e["ref"]


def test_corruptions_random_blocks_and_truncations():
    seen = {"kinds": set(), "stages": set()}
    errs = 0
    for blocks in bc.corrupted_stories():
        d, t = hpack_ref.Decoder(), hpack_ref.Decoder()
        for w in blocks:
            errs += isinstance(_both(w, d, t, seen), tuple)
    assert errs > 20
    rnd = bc.random_blocks()
    assert len(rnd) == 3000
    for w in rnd:
        _both(w, hpack_ref.Decoder(), hpack_ref.Decoder(), seen)
    g = load("rfc7541_blocks.json")
    for seq in g["sequences"]:
        for k, b in enumerate(seq["blocks"]):
            w = bytes.fromhex(b["wire"])
            for cut in range(len(w)):
                d, t = hpack_ref.Decoder(), hpack_ref.Decoder()
                for x in (d, t):
                    if seq["max_table_size"] is not None:
                        x.set_max_table_size(seq["max_table_size"])
                    for prev in seq["blocks"][:k]:
                        x.decode(bytes.fromhex(prev["wire"]))
                _both(w[:cut], d, t, seen)
    assert len(seen["kinds"]) >= 5, seen["kinds"]
    assert seen["stages"] == {bc.ST_INDEX, bc.ST_NAME, bc.ST_VALUE}


def test_placed_cases_reach_their_edges():
    cases = bc.placed()
    assert len(cases) >= 256 + 70
    seen = {"kinds": set(), "stages": set()}
    names = set()
    for name, block, expect in cases:
        assert name not in names
        names.add(name)
        fields, strings = bc.ref_scan(block)
        bc.check_expect(name, block, fields, strings, expect)
        for f in fields:  # the record's own invariants
            assert f.nstr <= 2 and (f.kind in bc._IS_LIT or f.nstr == 0)
            assert strings[f.str : f.str + f.nstr] == sorted(strings[f.str : f.str + f.nstr])
        _both(block, hpack_ref.Decoder(), hpack_ref.Decoder(), seen)
    assert seen["stages"] == {bc.ST_INDEX, bc.ST_NAME, bc.ST_VALUE}
    # the precedence cases mean what they say
    by_name = {n: b for n, b, _ in cases}
    assert _both(by_name["bad Huffman name, value cut short"], hpack_ref.Decoder(), hpack_ref.Decoder())[0] == "StringDecodingError"
    assert _both(by_name["bad Huffman name, value cut short"], hpack_ref.Decoder(), hpack_ref.Decoder())[1][0] == "HuffmanDecoderError"
    assert _both(by_name["size update last"], hpack_ref.Decoder(), hpack_ref.Decoder()) == ("SizeUpdateAtEnd", None)
    # an indexed name out of bounds beats the value's framing error
    assert _both(b"\x7f\x00\x05ab", hpack_ref.Decoder(), hpack_ref.Decoder()) == ("HeaderIndexOutOfBounds", None)
    assert len(bc.rfc_prefixes()) > 300
