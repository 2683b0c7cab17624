"""hpk_hdec_decode_blocks with the apply on the device (HuffmanCodec.set_block_apply("device")): the three settings of
one codec (host scan, device scan, device apply) on the corpora of test_gpu_blocks_device.py, each on fresh decoders,
must give the oracle's results per block and leave the same decoders: equal table_size() and equal table contents,
read on the host afterwards by decoding one block of the indexed fields 62 .. 61 + count per decoder. The device-apply
setting runs scan_blocks' kernels, decode_strings' pipeline and hpk_apply_blocks' kernel, carries every decoder's
table to the device and back, and falls back to the host apply for a whole call when a block is deferred."""

import ctypes

import pytest

import blocks_apply_cases as ac
import blocks_scan_cases as bc
from hpk_util import hpack_ref, load

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SETTINGS = (("host", "host"), ("device", "host"), ("host", "device"))  # (scan, apply); the apply setting overrides the scan's


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU)")
    from loona_amd import HuffmanCodec

    c = HuffmanCodec(0, stream=torch.cuda.current_stream())
    yield c
    c.set_block_scan("host")
    c.set_block_apply("host")
    c.close()


@pytest.fixture(scope="module")
def ring():
    from loona_amd import _lib

    r, c, w = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    assert _lib.lib().hpk_test_blkapply_geometry(ctypes.byref(r), ctypes.byref(c), ctypes.byref(w)) == _lib.HPK_E_OK
    return r.value


def choose(codec, setting):
    codec.set_block_scan(setting[0])
    codec.set_block_apply(setting[1])


def _ref(dec, wire):
    from loona_amd import hpack

    try:
        return dec.decode(wire)
    except hpack_ref.DecoderError as e:
        return hpack.DecoderError(e.kind, e.detail)


def contents(decs):
    """every decoder's table, read on the host: one block of the indexed fields 62 .. 61 + count each"""
    from loona_amd import hpack

    pairs = [(d, b"".join(ac.indexed(62 + i) for i in range(d.table_size()[1]))) for d in decs]
    return hpack.decode_blocks(pairs, None)


def three_settings(codec, stories, setup=None, calls=1, want=None, settings=None):
    """stories: [[block]], one decoder per story, in `calls` decode_blocks calls (story k's blocks cut into `calls`
    runs). settings: a (scan, apply) pair per call, else each of the three for all calls. Every run is on fresh
    decoders and must give the oracle's results and leave the first run's table sizes and contents. -> the results"""
    from loona_amd import hpack

    refs = []
    if want is None:
        refs = [hpack_ref.Decoder() for _ in stories]
        for k, r in enumerate(refs):
            if setup:
                setup(k, r)
        want = [[_ref(refs[k], w) for w in blocks] for k, blocks in enumerate(stories)]
    seen = []
    for plan in ([settings] if settings else [[s] * calls for s in SETTINGS]):
        decs = [hpack.Decoder() for _ in stories]
        for k, d in enumerate(decs):
            if setup:
                setup(k, d)
        got = [[] for _ in stories]
        for c in range(calls):
            choose(codec, plan[c])
            pairs, where = [], []
            for k, blocks in enumerate(stories):
                lo, hi = len(blocks) * c // calls, len(blocks) * (c + 1) // calls
                for w in blocks[lo:hi]:
                    pairs.append((decs[k], w))
                    where.append(k)
            for k, res in zip(where, hpack.decode_blocks(pairs, codec)):
                got[k].append(res)
        for k in range(len(stories)):
            assert got[k] == want[k], (plan[0], k, [w.hex() for w in stories[k]][:4])
        seen.append(([d.table_size() for d in decs], contents(decs)))
        assert seen[-1] == seen[0], plan
    choose(codec, SETTINGS[0])
    for k, r in enumerate(refs):
        assert seen[0][0][k][:2] == (r.dynamic.size, len(r.dynamic.table)), k
        assert seen[0][1][k] == r.dynamic.table, k
    return want


def test_set_block_apply_arguments(codec):
    from loona_amd import _lib

    with pytest.raises(ValueError):
        codec.set_block_apply("gpu")
    assert _lib.lib().hpk_ctx_set_block_apply(codec._h, 2) == _lib.HPK_E_INVAL
    assert _lib.lib().hpk_ctx_set_block_apply(codec._h, -1) == _lib.HPK_E_INVAL
    assert _lib.lib().hpk_ctx_set_block_apply(None, 1) == _lib.HPK_E_INVAL
    codec.set_block_apply("device")
    codec.set_block_apply("host")


def test_interop_stories_one_call(codec):
    stories = [[bytes.fromhex(c["wire"]) for c in story["cases"]] for _, story in bc.stories()]
    heads = [[[(n.encode(), v.encode()) for n, v in c["headers"]] for c in story["cases"]] for _, story in bc.stories()]
    three_settings(codec, stories, want=heads)
    assert sum(len(s) for s in stories) > 16000


def test_corrupted_stories_carry_their_tables(codec):
    from loona_amd import hpack

    want = three_settings(codec, bc.corrupted_stories())
    assert sum(isinstance(x, hpack.DecoderError) for s in want for x in s) > 20


def test_random_blocks_and_placed_cases(codec):
    """3331 decoders in one call; three of them defer (a size update above the ring), so this call's device-apply
    run is answered by the host apply as a whole"""
    from loona_amd import hpack

    blocks = bc.random_blocks() + [b for _, b, _ in bc.placed()]
    want = three_settings(codec, [[w] for w in blocks])
    kinds = {(x.kind, x.detail if not isinstance(x.detail, tuple) else x.detail[0]) for (x,) in want
             if isinstance(x, hpack.DecoderError)}
    assert len(kinds) >= 5
    (a,), (b,), (c,) = three_settings(codec, [[b"\x40" + bc.BAD_HUFF_NAME + b"\x05ab"], [b"\x7f\x00\x05ab"], [b"\x82\x20"]])
    assert a.kind == "StringDecodingError" and a.detail[0] == "HuffmanDecoderError"
    assert b.kind == "HeaderIndexOutOfBounds" and c.kind == "SizeUpdateAtEnd"


def test_the_applys_placed_cases(codec, ring):
    """blocks_apply_cases.placed() through the decoder path: the tables set up through the decoders' own calls"""
    cases = ac.placed(ring, 64)

    def setup(k, dec):
        tab = cases[k][1]
        for n, v in reversed(tab.entries):  # oldest first
            dec.decode(ac.lit_incr(n, v))
        dec.set_max_table_size(tab.max_size)
        if tab.max_allowed is not None:
            if isinstance(dec, hpack_ref.Decoder):
                dec.max_allowed_table_size = tab.max_allowed
            else:
                dec.set_max_allowed_table_size(tab.max_allowed)

    assert len(cases) > 30
    three_settings(codec, [blocks for _, _, blocks, _ in cases], setup)


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

    want = three_settings(codec, stories, setup)
    assert sum(isinstance(x, hpack.DecoderError) for (x,) in want) > 50


def test_calls_that_switch_setting_carry_state(codec):
    stories = [[bytes.fromhex(c["wire"]) for c in story["cases"]] for _, story in list(bc.stories())[:24]]
    h, s, a = SETTINGS
    three_settings(codec, stories, calls=2, settings=[a, h])
    three_settings(codec, stories, calls=2, settings=[s, a])
    three_settings(codec, stories, calls=2, settings=[a, a])
    corrupted = bc.corrupted_stories(seed=9, nstories=12)
    three_settings(codec, corrupted, calls=3, settings=[a, s, a])
    three_settings(codec, corrupted, calls=3, settings=[h, a, a])
    three_settings(codec, corrupted, calls=3)


def test_one_deferred_decoder_in_a_call(codec, ring):
    """one decoder's second block raises its table above what the ring holds: the whole call's answers still equal
    the host's, the other decoders' included, and a later call with that table set is answered too"""
    big = 32 * ring + 1
    stories = [[bytes.fromhex(c["wire"]) for c in story["cases"][:6]] for _, story in list(bc.stories())[:5]]
    stories.insert(2, [ac.lit_incr(b"a", b"1"), ac.size_update(big) + ac.lit_incr(b"b", b"2"), ac.indexed(62) + ac.indexed(63)])
    three_settings(codec, stories)
    three_settings(codec, stories, calls=3)  # (the third call starts with max_size above 32 * ring)


def test_no_blocks_and_empty_blocks(codec):
    from loona_amd import hpack

    choose(codec, ("host", "device"))
    assert hpack.decode_blocks([], codec) == []
    d = hpack.Decoder()
    assert hpack.decode_blocks([(d, b""), (hpack.Decoder(), b""), (d, b"")], codec) == [[], [], []]
    assert hpack.decode_blocks([(d, ac.lit_incr(b"k", b"v")), (d, b""), (d, ac.indexed(62))], codec) == [[(b"k", b"v")], [], [(b"k", b"v")]]
    choose(codec, SETTINGS[0])


def test_h2_frames_replay_under_the_setting(codec):
    """the hpk_h2_read_frames replay of test_gpu.py (every interop story as HEADERS + CONTINUATION frames over
    several calls) with the apply on the device"""
    from test_h2 import replay

    from loona_amd import h2

    choose(codec, ("host", "device"))
    assert replay(codec, seed=11) > 10000
    c = h2.Connection()
    r = h2.read_frames([c], [h2.frame(0x1, 0x5, 1, b"\x40")], codec)
    assert r.errors == ["HpackDecodingError"] and h2.error_code(r.errors[0]) == "COMPRESSION_ERROR"
    (blk,) = r.blocks
    assert blk[3].kind == "IntegerDecodingError"
    choose(codec, SETTINGS[0])


def _raw_call(codec, pairs):
    """hpk_hdec_decode_blocks as the C ABI returns it -> (n_headers, [block results], [header records], arena)"""
    import numpy as np

    from loona_amd import _lib

    L = _lib.lib()
    off = np.concatenate([[0], np.cumsum([len(b) for _, b in pairs])]).astype(np.uint32)
    blob = np.frombuffer(b"".join(b for _, b in pairs), dtype=np.uint8).copy()
    decs = (ctypes.c_void_p * len(pairs))(*[d._h for d, _ in pairs])
    out = _lib.BlocksOut()
    assert L.hpk_hdec_decode_blocks(codec._h, decs, blob.ctypes.data, off.ctypes.data, len(pairs), ctypes.byref(out)) == 0
    try:
        blocks = [(r.first_header, r.n_headers, r.error, r.detail) for r in (out.blocks[b] for b in range(out.n_blocks))]
        heads = [(h.name_off, h.name_len, h.value_off, h.value_len) for h in (out.headers[j] for j in range(out.n_headers))]
        return out.n_headers, blocks, heads, ctypes.string_at(out.arena, out.arena_len)
    finally:
        L.hpk_blocks_out_free(ctypes.byref(out))


def test_the_output_layout_the_header_states(codec, ring):
    """what hpk.h promises of the device-apply path's output, which also shows that the device applied: the header
    array is the field total long, first_header is field_off[b], records that no block covers are zero, and the
    arena begins with the static text; a call with a deferred block has the host apply's layout instead"""
    from loona_amd import batch, hpack

    text, _ = batch.static_table()
    blocks = [ac.size_update(100) + ac.indexed(2) + ac.lit_incr(b"k", b"v"), ac.indexed(3) + ac.indexed(99) + ac.indexed(4),
              ac.indexed(62)]
    choose(codec, ("host", "device"))
    d = hpack.Decoder()
    n, res, heads, arena = _raw_call(codec, [(d, w) for w in blocks])
    assert n == 7 and res == [(0, 2, 0, 0), (3, 1, 1, 0), (6, 1, 0, 0)]
    assert heads[2] == (0, 0, 0, 0) and heads[4] == (0, 0, 0, 0) and heads[5] == (0, 0, 0, 0)
    assert arena.startswith(text) and arena[len(text) :] == b"kv"
    assert d.table_size() == (34, 1, 100)
    # the carried-in entry's bytes lie behind the static text in the next call's arena
    n, res, heads, arena = _raw_call(codec, [(d, ac.indexed(62) + ac.lit_plain(62, b"w"))])
    assert n == 2 and res == [(0, 2, 0, 0)] and arena == text + b"kv" + b"w"
    assert heads[0] == (len(text), 1, len(text) + 1, 1) and heads[1] == (len(text), 1, len(text) + 2, 1)
    # a deferring size update: the host apply answers, with its own compact layout
    n, res, heads, arena = _raw_call(codec, [(d, ac.size_update(32 * ring + 1) + ac.indexed(62))])
    assert n == 1 and res == [(0, 1, 0, 0)] and arena == b"kv"
    choose(codec, ("device", "host"))
    n, res, heads, arena = _raw_call(codec, [(hpack.Decoder(), w) for w in blocks[:1]])
    assert n == 2 and res == [(0, 2, 0, 0)]
    choose(codec, SETTINGS[0])
