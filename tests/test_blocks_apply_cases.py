"""blocks_apply_cases.ref_apply pinned to the oracle (no GPU, no library).

ref_apply applies blocks_scan_cases.ref_scan's records and hpack_ref's decoded strings against a table of its own,
in the order hpk_hdec.cpp's apply_block states. Here, with a ring too large to defer anything, it must
reproduce hpack_ref.Decoder on every corpus of blocks_apply_cases.corpora(): the headers of a block that decodes,
the first error of one that does not, and after every block the table, entry by entry, and its limit. The placed
cases must also reach the edges they name, and the deferral rule must give the counts worked out for the issue."""

import blocks_apply_cases as ac
import blocks_scan_cases as bc
from hpk_util import hpack_ref

NO_DEFERRAL = 1 << 24


def oracle_for(tab):
    d = hpack_ref.Decoder()
    d.dynamic.table = list(tab.entries)
    d.dynamic.size = tab.size
    d.dynamic.max_size = tab.max_size
    d.max_allowed_table_size = tab.max_allowed
    return d


def pin(decoders, seen=None):
    """every decoder block by block through the oracle and through ref_apply -> blocks checked"""
    n = 0
    for tab, blocks in ac.fresh(decoders):
        tab.cap = None  # (no ring: nothing is deferred here)
        dec = oracle_for(tab)
        for w in blocks:
            try:
                want = dec.decode(w)
            except hpack_ref.DecoderError as e:
                want = (e.kind, e.detail)
            ((res,), applied), = ac.ref_apply([(tab, [w])], NO_DEFERRAL)
            headers, error, detail = res
            assert applied == 1
            got = headers if error == 0 else ac.as_decoder_error(error, detail)
            assert got == want, (w.hex(), got, want)
            assert tab.entries == dec.dynamic.table and tab.size == dec.dynamic.size, w.hex()
            assert tab.max_size == dec.dynamic.max_size, w.hex()
            if seen is not None and error:
                seen.add(error)
            n += 1
    return n


def test_interop_stories():
    c = ac.corpora()
    assert len(c["interop"]) == 159
    assert pin(c["interop"]) > 16000


def test_corrupted_random_and_truncated_blocks():
    c = ac.corpora()
    seen = set()
    assert pin(c["corrupted"], seen) + pin(c["corrupted9"], seen) > 500
    assert pin(c["random"], seen) == 3331
    assert pin(c["rfc"], seen) > 300
    assert {ac.E_OOB, 2, 4, 6, ac.E_HUFFMAN, ac.E_SU_AT_END} <= seen, seen


def test_placed_cases_reach_their_edges():
    cases = ac.placed()
    seen = set()
    assert pin([(tab, blocks) for _, tab, blocks, _ in cases], seen) > 150
    assert {ac.E_OOB, 4, ac.E_HUFFMAN, ac.E_INVALID_MAX, ac.E_SU_AT_END} <= seen, seen
    names = set()
    for name, tab, blocks, expect in cases:
        assert name not in names
        names.add(name)
        t = tab.copy()
        ((results, applied),) = ac.ref_apply([(t, blocks)], 2048)
        ac.check_expect(name, t, results, applied, expect)
        assert len(results) == len(blocks) and all(e == ac.E_DEFERRED for _, e, _ in results[applied:])
    # the geometry moves the cases with it
    for ring, chunk in ((128, 64), (256, 32)):
        for name, tab, blocks, expect in ac.placed(ring, chunk):
            t = tab.copy()
            ((results, applied),) = ac.ref_apply([(t, blocks)], ring)
            ac.check_expect(name, t, results, applied, expect)


def test_deferral_counts():
    """what the issue states: no interop or corrupted story defers at any ring from 128 records up (their largest
    size update is 2730, below 4096), and of the 3331 random and placed blocks 5 defer at lim = 128 and 3 from 256"""
    c = ac.corpora()
    for name in ("interop", "corrupted", "corrupted9"):
        for (_, applied), (_, blocks) in zip(ac.ref_apply(ac.fresh(c[name]), 128), c[name]):
            assert applied == len(blocks), name
    biggest = max((f.index for _, blocks in c["interop"] for w in blocks for f in bc.ref_scan(w)[0] if f.kind == bc.SIZE_UPDATE),
                  default=0)
    assert biggest == 2730
    for lim, want in ((128, 5), (256, 3), (2048, 3)):
        assert sum(applied == 0 for _, applied in ac.ref_apply(ac.fresh(c["random"]), lim)) == want, lim


def test_a_story_wraps_any_ring():
    c = ac.corpora()
    most = max(sum(f.kind == bc.LIT_INCR for w in blocks for f in bc.ref_scan(w)[0]) for _, blocks in c["interop"])
    assert most == 2494
