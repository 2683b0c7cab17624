"""hpack.encode_blocks with the table logic on the device (HuffmanCodec.set_block_plan("device"): hpk_plan_blocks'
kernels, the ordered pack, the string-literal encode) against the default path and hpack_ref.Encoder, byte for byte:
the blocks, the encoders' table sizes, and a follow-up block per encoder, which only comes out right if the tables
rebuilt from what the device sent back are the reference's."""

import ctypes

import pytest

import blocks_plan_cases as pc
from hpk_util import hpack_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU)")
    from loona_amd import HuffmanCodec

    c = HuffmanCodec(0, stream=torch.cuda.current_stream())
    yield c
    c.set_block_plan("host")
    c.close()


@pytest.fixture(scope="module")
def ring():
    from loona_amd import _lib

    v = [ctypes.c_uint32() for _ in range(4)]
    assert _lib.lib().hpk_test_blkplan_geometry(*[ctypes.byref(x) for x in v]) == _lib.HPK_E_OK
    return v[0].value


def lists(ring):
    """[(max_size, [block])]: every fourth interop story, the random lists and the placed cases that start from an
    empty table the ring can hold"""
    c = pc.corpora(ring, 64, 64)
    out = [(4096, blocks) for _, blocks, _ in c["interop"][::4]]
    out += [(tab.max_size, blocks) for tab, blocks, _ in c["random"]]
    out += [(tab.max_size, blocks) for tab, blocks, _ in c["placed"] if not tab.entries and tab.max_size <= 32 * ring and blocks]
    return out


def encoders(cases, huffman, cls):
    encs = []
    for max_size, _ in cases:
        e = cls(huffman=huffman)
        if max_size != 4096:
            e.set_max_table_size(max_size)
        encs.append(e)
    return encs


def interleaved(encs, cases, lo=0, hi=None):
    """[(encoder, block)]: the encoders' blocks lo .. hi position by position, so that the lists interleave"""
    where = sorted((k, e) for e, (_, blocks) in enumerate(cases) for k in range(len(blocks))[lo:hi])
    return [(encs[e], cases[e][1][k]) for k, e in where], where


def answered(codec):
    """hpk_henc_encode_blocks calls of this codec that the device-plan path answered (hpk_test_plan_calls)"""
    from loona_amd import _lib

    return _lib.lib().hpk_test_plan_calls(codec._h)


FOLLOW = [(b":method", b"GET"), (b"x-follow", b"up"), (b"x-0", b"v1"), (b"x-follow", b"up"), (b"cookie", b"a=b")]


def ref_size(r):
    return r.dynamic.size, len(r.dynamic.table), r.dynamic.max_size


@pytest.mark.parametrize("huffman", [False, True])
def test_both_settings_against_the_reference(codec, ring, huffman):
    from loona_amd import hpack

    cases = lists(ring)
    assert len(cases) > 350
    refs = encoders(cases, huffman, hpack_ref.Encoder)
    rpairs, where = interleaved(refs, cases)
    want = [r.encode(blk) for r, blk in rpairs]
    assert len(want) > 3000
    seen = {}
    for kind in ("host", "device"):
        codec.set_block_plan(kind)
        encs = encoders(cases, huffman, hpack.Encoder)
        n0 = answered(codec)
        got = hpack.encode_blocks(interleaved(encs, cases)[0], codec)
        assert got == want, kind
        assert [e.table_size() for e in encs] == [ref_size(r) for r in refs], kind
        seen[kind] = hpack.encode_blocks([(e, FOLLOW) for e in encs], codec)  # proves the rebuilt tables
        assert answered(codec) - n0 == (2 if kind == "device" else 0), kind  # which path answered the two calls
    assert seen["host"] == seen["device"] == [r.encode(FOLLOW) for r in refs]
    # and the blocks decode back, one decoder per encoder
    decs = [hpack.Decoder() for _ in cases]
    part = [(k, e) for k, e in where if cases[e][0] == 4096][:3000]
    index = {w: i for i, w in enumerate(where)}
    back = hpack.decode_blocks([(decs[e], want[index[(k, e)]]) for k, e in part], codec)
    assert back == [cases[e][1][k] for k, e in part]


def test_calls_that_switch_the_setting(codec, ring):
    from loona_amd import _lib, hpack

    with pytest.raises(ValueError):
        codec.set_block_plan("gpu")
    assert _lib.lib().hpk_ctx_set_block_plan(codec._h, 2) == _lib.HPK_E_INVAL  # (and the setting stays what it was)

    cases = [(m, blocks) for m, blocks in lists(ring)[:60] if len(blocks) >= 3]
    assert len(cases) > 30
    refs = encoders(cases, True, hpack_ref.Encoder)
    encs = encoders(cases, True, hpack.Encoder)
    for call, kind in enumerate(("device", "host", "device")):
        codec.set_block_plan(kind)
        lo, hi = (call, call + 1) if call < 2 else (2, None)
        want = [r.encode(blk) for r, blk in interleaved(refs, cases, lo, hi)[0]]
        assert hpack.encode_blocks(interleaved(encs, cases, lo, hi)[0], codec) == want, call
        assert [e.table_size() for e in encs] == [ref_size(r) for r in refs], call


def test_an_encoder_the_ring_cannot_hold_sends_the_call_to_the_host_path(codec, ring):
    from loona_amd import hpack

    cases = [(4096, [[(b"x-a", b"1"), (b"x-b", b"2")], [(b"x-a", b"1")]]), (32 * ring + 1, [[(b"x-c", b"3"), (b"x-c", b"3")]]),
             (32 * ring, [[(b"x-d", b"4")]])]
    refs = encoders(cases, False, hpack_ref.Encoder)
    want = [r.encode(blk) for r, blk in interleaved(refs, cases)[0]]
    codec.set_block_plan("device")
    encs = encoders(cases, False, hpack.Encoder)
    n0 = answered(codec)
    assert hpack.encode_blocks(interleaved(encs, cases)[0], codec) == want
    assert answered(codec) == n0  # the host path answered
    assert [e.table_size() for e in encs] == [ref_size(r) for r in refs]
    # without the large one the same call runs on the device, with the same bytes
    encs = encoders(cases, False, hpack.Encoder)
    pairs, where = interleaved(encs, cases)
    keep = [i for i, (_, e) in enumerate(where) if e != 1]
    assert hpack.encode_blocks([pairs[i] for i in keep], codec) == [want[i] for i in keep]
    assert answered(codec) == n0 + 1


def test_the_default_setting_is_host(ring):
    """a codec that never had set_block_plan called. Raw encoders never reach a Huffman batch on the host path, so an
    injected batch failure is not consumed there and the call succeeds; the device path consumes it before any upload"""
    from loona_amd import HuffmanCodec, _lib, hpack

    cases = lists(ring)[40:60]
    refs = encoders(cases, False, hpack_ref.Encoder)
    want = [r.encode(blk) for r, blk in interleaved(refs, cases)[0]]
    L = _lib.lib()
    with HuffmanCodec(0, stream=torch.cuda.current_stream()) as fresh:
        try:
            L.hpk_test_fail_batches(1)
            encs = encoders(cases, False, hpack.Encoder)
            assert hpack.encode_blocks(interleaved(encs, cases)[0], fresh) == want
            assert answered(fresh) == 0
            fresh.set_block_plan("device")
            encs = encoders(cases, False, hpack.Encoder)
            with pytest.raises(RuntimeError, match=r"\(-3\)"):  # the injection left over from above
                hpack.encode_blocks(interleaved(encs, cases)[0], fresh)
            assert answered(fresh) == 0 and all(e.table_size()[:2] == (0, 0) for e in encs)
            assert hpack.encode_blocks(interleaved(encs, cases)[0], fresh) == want
            assert answered(fresh) == 1
            fresh.set_block_plan("host")
            encs = encoders(cases, False, hpack.Encoder)
            assert hpack.encode_blocks(interleaved(encs, cases)[0], fresh) == want
            assert answered(fresh) == 1
        finally:
            L.hpk_test_fail_batches(0)


def test_a_failed_batch_leaves_every_encoder_as_it_was(codec, ring):
    from loona_amd import _lib, hpack

    cases = lists(ring)[30:70]  # stories and random lists
    refs = encoders(cases, True, hpack_ref.Encoder)
    encs = encoders(cases, True, hpack.Encoder)
    codec.set_block_plan("device")
    first = interleaved(encs, cases, 0, 1)[0]
    assert hpack.encode_blocks(first, codec) == [r.encode(blk) for r, blk in interleaved(refs, cases, 0, 1)[0]]
    before = [e.table_size() for e in encs]
    assert sum(n for _, n, _ in before) > 10  # there is state to lose
    rest = interleaved(encs, cases, 1, None)[0]
    _lib.lib().hpk_test_fail_batches(1)
    try:
        n0 = answered(codec)
        with pytest.raises(RuntimeError, match=r"\(-3\)"):
            hpack.encode_blocks(rest, codec)
        assert answered(codec) == n0
    finally:
        _lib.lib().hpk_test_fail_batches(0)
    assert [e.table_size() for e in encs] == before
    want = [r.encode(blk) for r, blk in interleaved(refs, cases, 1, None)[0]]
    assert hpack.encode_blocks(rest, codec) == want  # the retried call
    assert [e.table_size() for e in encs] == [ref_size(r) for r in refs]
    assert hpack.encode_blocks([(e, FOLLOW) for e in encs], codec) == [r.encode(FOLLOW) for r in refs]
