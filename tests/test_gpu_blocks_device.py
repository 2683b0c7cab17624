"""hpk_hdec_decode_blocks with the scan on the device (HuffmanCodec.set_block_scan("device")): per block the headers
or the first error must equal hpack_ref.Decoder's, and the host-scan path's of the same codec on the same input,
decoder states included. The device path tokenises with hpk_scan_blocks' kernels, decodes every listed string with
decode_strings' pipeline and applies the public hpk_field records on the host."""

import pytest

import blocks_scan_cases as bc
from hpk_util import hpack_ref, load

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU)")
    from loona_amd import HuffmanCodec

    c = HuffmanCodec(0, stream=torch.cuda.current_stream())
    yield c
    c.set_block_scan("host")
    c.close()


def _ref(dec, wire):
    from loona_amd import hpack

    try:
        return dec.decode(wire)
    except hpack_ref.DecoderError as e:
        return hpack.DecoderError(e.kind, e.detail)


def both_paths(codec, stories, setup=None, calls=1, want=None):
    """stories: [[block]], one decoder per story. The blocks of all stories in `calls` decode_blocks calls (story
    k's blocks cut into `calls` runs), once per scan setting on fresh decoders; both must give the oracle's
    results and leave the same table sizes. setup(k, decoder): the story's decoder before its first block, for the
    library's and the oracle's alike. want: the results, where a fixture holds what the oracle gives (the interop
    stories' header lists, which tests/test_blocks_scan_cases.py checks against hpack_ref.Decoder); else the oracle
    runs here and its table sizes are compared too. -> the expected results"""
    from loona_amd import hpack

    refs = []
    if want is None:
        refs = [hpack_ref.Decoder() for _ in stories]
        for k, r in enumerate(refs):
            if setup:
                setup(k, r)
        want = [[_ref(refs[k], w) for w in blocks] for k, blocks in enumerate(stories)]
    sizes = {}
    for kind in ("device", "host"):
        codec.set_block_scan(kind)
        decs = [hpack.Decoder() for _ in stories]
        for k, d in enumerate(decs):
            if setup:
                setup(k, d)
        got = [[] for _ in stories]
        for c in range(calls):
            pairs, where = [], []
            for k, blocks in enumerate(stories):
                lo, hi = len(blocks) * c // calls, len(blocks) * (c + 1) // calls
                for w in blocks[lo:hi]:
                    pairs.append((decs[k], w))
                    where.append(k)
            for k, res in zip(where, hpack.decode_blocks(pairs, codec)):
                got[k].append(res)
        for k in range(len(stories)):
            assert got[k] == want[k], (kind, k, [w.hex() for w in stories[k]][:4])
        sizes[kind] = [d.table_size() for d in decs]
    assert sizes["device"] == sizes["host"]
    for k, r in enumerate(refs):
        assert sizes["device"][k][:2] == (r.dynamic.size, len(r.dynamic.table)), k
    return want


def test_set_block_scan_arguments(codec):
    from loona_amd import _lib

    with pytest.raises(ValueError):
        codec.set_block_scan("gpu")
    assert _lib.lib().hpk_ctx_set_block_scan(codec._h, 2) == _lib.HPK_E_INVAL
    assert _lib.lib().hpk_ctx_set_block_scan(None, 1) == _lib.HPK_E_INVAL
    codec.set_block_scan("device")
    codec.set_block_scan("host")


def test_interop_stories_one_call(codec):
    stories = [[bytes.fromhex(c["wire"]) for c in story["cases"]] for _, story in bc.stories()]
    heads = [[[(n.encode(), v.encode()) for n, v in c["headers"]] for c in story["cases"]] for _, story in bc.stories()]
    both_paths(codec, stories, want=heads)
    assert sum(len(s) for s in stories) > 16000


def test_corrupted_stories_carry_their_tables(codec):
    from loona_amd import hpack

    want = both_paths(codec, bc.corrupted_stories())
    assert sum(isinstance(x, hpack.DecoderError) for s in want for x in s) > 20


def test_random_blocks_and_placed_cases(codec):
    from loona_amd import hpack

    blocks = bc.random_blocks() + [b for _, b, _ in bc.placed()]
    want = both_paths(codec, [[w] for w in blocks])
    kinds = {(x.kind, x.detail if not isinstance(x.detail, tuple) else x.detail[0]) for (x,) in want
             if isinstance(x, hpack.DecoderError)}
    assert len(kinds) >= 5
    # the precedences the issue names: a Huffman error in a name beats the value's framing error; an indexed name
    # out of bounds beats the value's errors; SizeUpdateAtEnd comes last
    (a,), (b,), (c,) = both_paths(codec, [[b"\x40" + bc.BAD_HUFF_NAME + b"\x05ab"], [b"\x7f\x00\x05ab"], [b"\x82\x20"]])
    assert a.kind == "StringDecodingError" and a.detail[0] == "HuffmanDecoderError"
    assert b.kind == "HeaderIndexOutOfBounds" and c.kind == "SizeUpdateAtEnd"


def test_every_truncation_of_rfc_blocks(codec):
    from loona_amd import hpack

    g = load("rfc7541_blocks.json")
    stories, prime = [], []
    for seq in g["sequences"]:
        for k, b in enumerate(seq["blocks"]):
            w = bytes.fromhex(b["wire"])
            for cut in range(len(w)):
                stories.append([w[:cut]])
                prime.append((seq["max_table_size"], [bytes.fromhex(p["wire"]) for p in seq["blocks"][:k]]))

    def setup(k, dec):
        size, before = prime[k]
        if size is not None:
            dec.set_max_table_size(size)
        for w in before:
            dec.decode(w)

    want = both_paths(codec, stories, setup)
    assert sum(isinstance(x, hpack.DecoderError) for (x,) in want) > 50


def test_two_calls_carry_state(codec):
    stories = [[bytes.fromhex(c["wire"]) for c in story["cases"]] for _, story in list(bc.stories())[:24]]
    both_paths(codec, stories, calls=2)
    both_paths(codec, bc.corrupted_stories(seed=9, nstories=12), calls=3)


def test_no_blocks_and_empty_blocks(codec):
    from loona_amd import hpack

    codec.set_block_scan("device")
    assert hpack.decode_blocks([], codec) == []
    assert hpack.decode_blocks([(hpack.Decoder(), b""), (hpack.Decoder(), b"")], codec) == [[], []]
    codec.set_block_scan("host")


def test_h2_frames_replay_both_settings(codec):
    """the hpk_h2_read_frames replay of test_gpu.py (every interop story as HEADERS + CONTINUATION frames over
    several calls): the same blocks and connection errors under both settings"""
    from test_h2 import replay

    from loona_amd import h2

    for kind in ("device", "host"):
        codec.set_block_scan(kind)
        assert replay(codec, seed=11) > 10000
        c = h2.Connection()
        r = h2.read_frames([c], [h2.frame(0x1, 0x5, 1, b"\x40")], codec)
        assert r.errors == ["HpackDecodingError"] and h2.error_code(r.errors[0]) == "COMPRESSION_ERROR"
        (blk,) = r.blocks
        assert blk[3].kind == "IntegerDecodingError"
