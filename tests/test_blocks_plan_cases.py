"""blocks_plan_cases.ref_plan, the model the emulation and the GPU tests of hpk_plan_blocks compare with, pinned to
hpack_ref.Encoder (no GPU needed): per block the items put together by the rule of hpk_encode_strings_packed
(encode_strings_cases.expected) equal Encoder.encode's bytes, with huffman False and True; the final table equals
the encoder's; and every placed case reaches the edge it names."""

import pytest

import blocks_plan_cases as pc
from hpk_util import hpack_ref

RING = 2048


def pinned(encoders):
    """ref_plan on copies against hpack_ref.Encoder primed with the same table -> the planned encoder count"""
    tabs = pc.fresh(encoders)
    got = pc.ref_plan(tabs, RING)
    planned = 0
    items, want = [], []
    for (results, n), (tab, blocks, huffman), (tab0, _, _) in zip(got, tabs, encoders):
        if n == 0 and blocks:  # deferred: the model leaves the table as it came
            assert all(r is None for r in results) and tab.entries == tab0.entries and tab.max_size == tab0.max_size
            continue
        planned += 1
        enc = hpack_ref.Encoder(huffman=huffman)
        enc.dynamic.max_size = tab0.max_size
        enc.dynamic.table = list(tab0.entries)
        enc.dynamic.size = tab0.size
        for blk, res in zip(blocks, results):
            want.append(enc.encode(blk))
            items.append([it for _, _, _, it in res])
            for (kind, index, prefix, it), (name, value) in zip(res, blk):
                assert it[0] == (pc.VERBATIM, prefix) and 1 <= len(prefix) <= 3
                assert (kind == pc.NEW_NAME) == (index == 0)
                assert {pc.INDEXED: prefix[0] >= 0x80, pc.NAME_INDEXED: prefix[0] < 0x10, pc.NEW_NAME: prefix == b"\x40"}[kind]
        assert enc.dynamic.table == tab.entries and enc.dynamic.size == tab.size and enc.dynamic.max_size == tab.max_size
    assert pc.assemble(items) == want
    return planned


@pytest.mark.parametrize("name", ["interop", "random", "placed"])
def test_ref_plan_matches_the_reference_encoder(name):
    encoders = pc.corpora(RING)[name]
    if name == "interop":
        assert len(encoders) == 159 and sum(len(b) for _, b, _ in encoders) > 16000
    assert pinned(encoders) >= len(encoders) - 3


def test_both_huffman_settings():
    """every interop story the other way round (the corpus alternates), and the random lists all raw and all coded"""
    c = pc.corpora(RING)
    flipped = [(tab, blocks, not huffman) for tab, blocks, huffman in c["interop"][::4]]
    assert pinned(flipped) == len(flipped)
    for huffman in (False, True):
        assert pinned([(tab, blocks, huffman) for tab, blocks, _ in c["random"]]) == len(c["random"])


def test_placed_cases_reach_their_edges():
    cases = pc.placed(RING, 64, 64)
    assert len(cases) >= 45
    encoders = pc.fresh([(tab, blocks, huffman) for _, tab, blocks, huffman, _ in cases])
    got = pc.ref_plan(encoders, RING)
    for (name, _, _, _, expect), (results, planned), (tab, _, _) in zip(cases, got, encoders):
        pc.check_expect(name, tab, results, planned, expect)
    kinds = {h[0] for results, _ in got for blk in results if blk for h in blk}
    assert kinds == {pc.INDEXED, pc.NAME_INDEXED, pc.NEW_NAME}
    assert max(len(h[2]) for results, _ in got for blk in results if blk for h in blk) == 3  # index 61 + ring: three octets


@pytest.mark.parametrize("calls", [2, 3])
def test_tables_carried_over_calls(calls):
    """the model fed its own tables call after call against one hpack_ref.Encoder per story that never stops"""
    stories, tabs = pc.carried(RING)
    refs = []
    for t, (_, h) in zip(tabs, stories):
        refs.append(hpack_ref.Encoder(huffman=h))
        refs[-1].set_max_table_size(t.max_size)
    for c in range(calls):
        part = [blocks[len(blocks) * c // calls : len(blocks) * (c + 1) // calls] for blocks, _ in stories]
        tabs = [pc.Table(t.entries, t.max_size) for t in tabs]  # laid out afresh, as a caller carries them
        got = pc.ref_plan([(t, p, h) for t, p, (_, h) in zip(tabs, part, stories)], RING)
        assert all(planned == len(p) for (_, planned), p in zip(got, part))
        assert pc.assemble([[it for _, _, _, it in blk] for res, _ in got for blk in res]) == [r.encode(blk) for r, p in zip(refs, part) for blk in p]
        assert [(t.entries, t.size) for t in tabs] == [(r.dynamic.table, r.dynamic.size) for r in refs]
    assert sum(len(t.entries) for t in tabs) > 0


def test_collisions_are_found():
    (a, b), (c, d) = pc.collisions()
    assert len({a, b, c, d}) == 4 and all(len(x) == 8 for x in (a, b, c, d))
