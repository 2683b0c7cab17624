"""hpk_h2_write_headers and h2.write_headers on the host (no GPU needed): the block encoder and the framing in one
call, with ctx = NULL, against hpack_ref's encoder followed by frames_write_cases.ref_write_frames."""

import ctypes
import random

import numpy as np
import pytest

import frames_cases as fc
import frames_write_cases as wc
from hpk_util import hpack_ref, load
from loona_amd import _lib, h2, hpack


def header_lists(limit=120):
    inter = load("interop.json.gz")
    out = []
    for enc in sorted(inter):
        for story in inter[enc][:3]:
            out.append([[(n.encode(), v.encode()) for n, v in c["headers"]] for c in story["cases"][:8]])
            if sum(len(s) for s in out) >= limit:
                return out
    return out


def tables(encs):
    return [e.table_size() for e in encs]


@pytest.mark.parametrize("huffman", [False, True])
def test_write_headers_matches_reference_encoder_and_model(huffman):
    rng = random.Random(2)
    stories = header_lists()
    encs = [hpack.Encoder(huffman=huffman) for _ in stories]
    refs = [hpack_ref.Encoder(huffman=huffman) for _ in stories]
    # the connections interleaved at random, each connection's blocks in their own order
    turns = [k for k, s in enumerate(stories) for _ in s]
    rng.shuffle(turns)
    nxt = [iter(s) for s in stories]
    seq = [(k, next(nxt[k])) for k in turns]
    sids = [(2 * i + 1) | (wc.ES_BIT if rng.random() < 0.4 else 0) for i in range(len(seq))]
    mfs = [rng.choice([1, 7, 16, 50, 16384, 0xFFFFFF]) for _ in seq]
    got = h2.write_headers([encs[k] for k, _ in seq], [hl for _, hl in seq], sids, mfs)
    want = [wc.ref_write_frames(refs[k].encode(hl), sid, m) for (k, hl), sid, m in zip(seq, sids, mfs)]
    assert got == want and len(seq) > 50
    assert tables(encs) == [(r.dynamic.size, len(r.dynamic.table), r.dynamic.max_size) for r in refs]
    # and the frame scan's model reads every block back
    for w, (k, hl), sid, m in zip(got, seq, sids, mfs):
        scan = fc.ref_scan_frames(fc.State(m), w, b"")
        assert [b[0] for b in scan.blocks] == [sid] and scan.consumed == len(w)


@pytest.mark.parametrize("bad", [0, 0x1000000, 0xFFFFFFFF])
def test_bad_max_frame_leaves_the_encoders_untouched(bad):
    stories = header_lists(30)
    encs = [hpack.Encoder(huffman=True) for _ in stories]
    h2.write_headers(encs, [s[0] for s in stories], [1] * len(encs), [16384] * len(encs))
    before = tables(encs)
    mfs = [16384] * len(encs)
    mfs[-1] = bad
    with pytest.raises(Exception):
        h2.write_headers(encs, [s[1] for s in stories], [3] * len(encs), mfs)
    assert tables(encs) == before
    # the same blocks go through afterwards as if the failed call had not been
    refs = [hpack_ref.Encoder(huffman=True) for _ in stories]
    for r, s in zip(refs, stories):
        r.encode(s[0])
    got = h2.write_headers(encs, [s[1] for s in stories], [3] * len(encs), [16384] * len(encs))
    assert got == [wc.ref_write_frames(r.encode(s[1]), 3, 16384) for r, s in zip(refs, stories)]


def test_c_abi_null_context_and_no_blocks():
    L = _lib.lib()
    out = _lib.HencOut()
    hoff = np.zeros(1, np.uint32)
    encs = (ctypes.c_void_p * 1)()
    assert L.hpk_h2_write_headers(None, encs, None, None, hoff.ctypes.data, 0, None, None, ctypes.byref(out)) == 0
    assert out.len == 0 and out.n_blocks == 0 and out.block_off[0] == 0
    L.hpk_henc_out_free(ctypes.byref(out))
    assert h2.write_headers([], [], [], []) == []


def test_empty_header_list_is_one_empty_headers_frame():
    e = hpack.Encoder()
    assert h2.write_headers([e], [[]], [5 | wc.ES_BIT], [16384]) == [bytes.fromhex("000000 01 05 00000005".replace(" ", ""))]
