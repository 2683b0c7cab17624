"""hpk_h2_write_headers with the framing on the device (HPK_FRAME_WRITE_DEVICE) beside the default host framing: the
same octets and the same encoders, hpk_test_frame_write_calls telling which path answered; the same with the table
logic on the device too (HPK_BLOCK_PLAN_DEVICE); and an injected failure of the device framing, which the host
framing answers because the encoders' tables are committed by then."""

import random

import pytest

import frames_write_cases as wc
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
    c.set_frame_write("host")
    c.set_block_plan("host")
    c.close()


@pytest.fixture(scope="module")
def work():
    """[(connection, header list)] interleaved, the stream words and the frame sizes"""
    inter = load("interop.json.gz")
    stories = [[[(n.encode(), v.encode()) for n, v in c["headers"]] for c in story["cases"][:10]]
               for enc in sorted(inter) for story in inter[enc][:8]]
    rng = random.Random(4)
    turns = [k for k, s in enumerate(stories) for _ in s]
    rng.shuffle(turns)
    nxt = [iter(s) for s in stories]
    seq = [(k, next(nxt[k])) for k in turns]
    sids = [(2 * i + 1) | (wc.ES_BIT if rng.random() < 0.4 else 0) for i in range(len(seq))]
    mfs = [rng.choice([1, 7, 16, 50, 16384, 0xFFFFFF]) for _ in seq]
    assert len(seq) > 100
    return len(stories), seq, sids, mfs


def calls(codec):
    from loona_amd import _lib

    return _lib.lib().hpk_test_frame_write_calls(codec._h)


def one_call(codec, work, huffman, ctx=True):
    from loona_amd import h2, hpack

    nconn, seq, sids, mfs = work
    encs = [hpack.Encoder(huffman=huffman) for _ in range(nconn)]
    before = calls(codec)
    got = h2.write_headers([encs[k] for k, _ in seq], [hl for _, hl in seq], sids, mfs, codec if ctx else None)
    return got, [e.table_size() for e in encs], calls(codec) - before


def reference(work, huffman):
    nconn, seq, sids, mfs = work
    refs = [hpack_ref.Encoder(huffman=huffman) for _ in range(nconn)]
    return [wc.ref_write_frames(refs[k].encode(hl), sid, m) for (k, hl), sid, m in zip(seq, sids, mfs)]


@pytest.mark.parametrize("plan", ["host", "device"])
@pytest.mark.parametrize("huffman", [False, True])
def test_both_framings_side_by_side(codec, work, huffman, plan):
    codec.set_block_plan(plan)
    codec.set_frame_write("host")
    host = one_call(codec, work, huffman)
    codec.set_frame_write("device")
    dev = one_call(codec, work, huffman)
    codec.set_frame_write("host")
    codec.set_block_plan("host")
    assert host[2] == 0 and dev[2] == 1
    assert dev[:2] == host[:2]
    assert host[0] == reference(work, huffman)
    assert one_call(codec, work, huffman, ctx=False)[:2] == host[:2]


def test_injected_failure_is_answered_by_the_host_framing(codec, work):
    from loona_amd import _lib

    codec.set_frame_write("host")
    host = one_call(codec, work, False)
    codec.set_frame_write("device")
    _lib.lib().hpk_test_fail_batches(1)  # raw encoders: no Huffman batch takes the count before the framing does
    try:
        dev = one_call(codec, work, False)
    finally:
        _lib.lib().hpk_test_fail_batches(0)
    assert dev[2] == 0 and dev[:2] == host[:2]
    again = one_call(codec, work, False)  # the count is used up: the device answers
    codec.set_frame_write("host")
    assert again[2] == 1 and again[:2] == host[:2]


def test_bad_max_frame_on_the_device_path(codec, work):
    from loona_amd import h2, hpack

    codec.set_frame_write("device")
    e = hpack.Encoder()
    before = e.table_size()
    with pytest.raises(RuntimeError):
        h2.write_headers([e], [[(b"x-a", b"b")]], [1], [0], codec)
    codec.set_frame_write("host")
    assert e.table_size() == before
