"""One codec, one stream's slot, every kind of call that stages through it, small then large then small again: the
slot's buffers regrow under the larger call (each kind's own staging buffer, and pk_tmp and the string decode's
scratch, which the kinds share) and are reused, larger than needed, by the smaller one after it. The kinds are
interleaved at every size, so each call finds the slot as another kind left it.

Host forms (3, 300, 3 items): the string-literal encode, the string-literal decode (the mirror and the two-array
form) and the block scan, against the answers tests/encode_strings_cases.py, tests/decode_strings_cases.py and
tests/blocks_scan_cases.py give (the C oracle and hpack_ref). Device block paths (1 block, the interop corpus's first
50, 1 block): decode_blocks with the scan, and with the scan and the apply, on the device, against the corpus's header
lists and the host path's table sizes; encode_blocks with the plan on the device against hpack_ref.Encoder and the
host path."""

import numpy as np
import pytest

import blocks_scan_cases as bc
import decode_strings_cases as dc
import encode_strings_cases as sc
from hpk_util import hpack_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ITEMS = (3, 300, 3)
BLOCKS = (1, 50, 1)


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU)")
    from loona_amd import HuffmanCodec

    c = HuffmanCodec(0, stream=torch.cuda.current_stream())
    yield c
    for setting in (c.set_block_scan, c.set_block_apply, c.set_block_plan):
        setting("host")
    c.close()


@pytest.fixture(scope="module")
def corpus():
    """the interop corpus's first 300 blocks: [(story, wire, headers)], a story's blocks in its order"""
    out = []
    for k, (_, story) in enumerate(bc.stories()):
        out += [(k, bytes.fromhex(c["wire"]), [(n.encode(), v.encode()) for n, v in c["headers"]]) for c in story["cases"]]
        if len(out) >= 300:
            return out[:300]
    raise AssertionError("the interop corpus has fewer than 300 blocks")


def strings_encode(codec, n, seed):
    strs, pol = sc.mixed_batch(n, 60, seed)
    x = sc.expected(strs, pol)
    ob, oo, ol, st = codec.encode_strings_host(x.blob, x.in_off, pol)
    assert not st.any() and np.array_equal(ol.astype(np.int64), x.out_len), ("strings encode", n)
    assert np.array_equal(oo.astype(np.int64), x.out_off) and np.array_equal(ob, x.flat), ("strings encode", n)


def strings_decode(codec, n, seed):
    b, strs = dc.mixed_batch(n, seed)
    x = dc.expected(b)
    assert not x.status.any() and x.flat.tobytes() == b"".join(strs)
    mirror = np.append(b.str_off, b.str_end[-1])
    for form, args in (("mirror", (mirror,)), ("two arrays", (b.str_off, b.str_end))):
        ob, oo, ol, co, st = codec.decode_strings_host(b.blob, *args)
        assert np.array_equal(st, x.status) and np.array_equal(ol.astype(np.int64), x.out_len), ("strings decode", form, n)
        assert np.array_equal(co.astype(np.int64), x.consumed) and np.array_equal(oo.astype(np.int64), x.out_off), ("strings decode", form, n)
        assert np.array_equal(ob, x.flat), ("strings decode", form, n)


def block_scan(codec, blocks):
    x = bc.expected_batch(blocks)
    f, foff, so, se, soff, st = codec.scan_blocks_host(x.blob, x.block_off)
    assert np.array_equal(foff, x.field_off) and np.array_equal(soff, x.str_blk_off) and not st.any(), ("block scan", len(blocks))
    assert np.array_equal(f, x.fields) and np.array_equal(so, x.str_off) and np.array_equal(se, x.str_end), ("block scan", len(blocks))


def blocks_decode(codec, part, scan, apply):
    """the part's blocks, a decoder per story, under the setting and on the host path: the corpus's headers, one state"""
    from loona_amd import hpack

    sizes = []
    for setting in ((scan, apply), ("host", "host")):
        codec.set_block_scan(setting[0])
        codec.set_block_apply(setting[1])
        decs = {k: hpack.Decoder() for k, _, _ in part}
        got = hpack.decode_blocks([(decs[k], wire) for k, wire, _ in part], codec)
        assert got == [heads for _, _, heads in part], (setting, len(part))
        sizes.append([d.table_size() for d in decs.values()])
    assert sizes[0] == sizes[1], (scan, apply, len(part))


def blocks_encode(codec, part):
    """the part's header lists, an encoder per story, with the plan on the device and on the host: hpack_ref's bytes"""
    from loona_amd import _lib, hpack

    refs = {k: hpack_ref.Encoder(huffman=k % 2 == 0) for k, _, _ in part}
    want = [refs[k].encode(heads) for k, _, heads in part]
    for kind in ("device", "host"):
        codec.set_block_plan(kind)
        encs = {k: hpack.Encoder(huffman=k % 2 == 0) for k, _, _ in part}
        n0 = _lib.lib().hpk_test_plan_calls(codec._h)
        assert hpack.encode_blocks([(encs[k], heads) for k, _, heads in part], codec) == want, (kind, len(part))
        assert _lib.lib().hpk_test_plan_calls(codec._h) - n0 == (kind == "device"), (kind, len(part))  # which path answered
        assert [e.table_size() for e in encs.values()] == [(r.dynamic.size, len(r.dynamic.table), r.dynamic.max_size) for r in refs.values()]


def test_small_large_small_with_the_kinds_interleaved(codec, corpus):
    for step, (n, nb) in enumerate(zip(ITEMS, BLOCKS)):
        strings_encode(codec, n, 10 + step)
        blocks_decode(codec, corpus[:nb], "device", "host")
        strings_decode(codec, n, 20 + step)
        blocks_encode(codec, corpus[:nb])
        block_scan(codec, [w for _, w, _ in corpus[:n]])
        blocks_decode(codec, corpus[:nb], "device", "device")


KINDS = {
    "strings encode": lambda c, corpus, big: strings_encode(c, ITEMS[big], 31),
    "strings decode": lambda c, corpus, big: strings_decode(c, ITEMS[big], 32),
    "block scan": lambda c, corpus, big: block_scan(c, [w for _, w, _ in corpus[: ITEMS[big]]]),
    "device scan": lambda c, corpus, big: blocks_decode(c, corpus[: BLOCKS[big]], "device", "host"),
    "device apply": lambda c, corpus, big: blocks_decode(c, corpus[: BLOCKS[big]], "device", "device"),
    "device plan": lambda c, corpus, big: blocks_encode(c, corpus[: BLOCKS[big]]),
}


@pytest.mark.parametrize("kind", list(KINDS))
def test_large_first_under_each_kind(corpus, kind):
    """A fresh codec whose first call is the kind's large one: pk_tmp and every other buffer the kind uses grow from
    nothing under it; then another kind's large call on the slot it left, and the kind's small one."""
    from loona_amd import HuffmanCodec

    other = list(KINDS)[(list(KINDS).index(kind) + 1) % len(KINDS)]
    with HuffmanCodec(0, stream=torch.cuda.current_stream()) as c:
        KINDS[kind](c, corpus, 1)
        KINDS[other](c, corpus, 1)
        KINDS[kind](c, corpus, 0)
