"""The packed string-literal encode's cases (encode_strings_cases.py) on the CPU: expected() is hpack_ref's
string literal, every placed case reaches the cut or edge it claims (the emit kernel cuts its tiles by
hpk_encode2's rule, encode_cases.tile_plan, on the representations' offsets with its own geometry), and the
calls refuse a NULL context."""

import ctypes

import numpy as np
import pytest

import encode_cases as ec
import encode_packed_cases as pc
import encode_strings_cases as sc
from encode_cases import HEAD
from hpk_util import hpack_ref


@pytest.fixture(scope="module")
def geo():
    return sc.geometry()


def literal(x, i):
    return x.flat[x.out_off[i] : x.out_off[i + 1]].tobytes()


def test_geometry(geo):
    assert geo.T % 16 == 0 and geo.I % 16 == 0 and geo.T and geo.Q and geo.P
    assert geo.T + 6 * geo.Q + 16 <= geo.I  # a tile of raw literals: the image never binds before the input


def test_expected_is_hpack_ref_string():
    strs, _ = sc.mixed_batch(400, 300, 20000)
    strs += sc.decision_edge()[0] + [b"", b"www.example.com"]
    for pol, enc in ((sc.AUTO, hpack_ref.Encoder(huffman=True)), (sc.RAW, hpack_ref.Encoder(huffman=False))):
        x = sc.expected(strs, sc.policies(len(strs), pol))
        for i, s in enumerate(strs):
            assert literal(x, i) == enc._string(s), (pol, i)
    x = sc.expected(strs, sc.policies(len(strs), sc.VERBATIM))
    assert x.flat.tobytes() == b"".join(strs) and np.array_equal(x.out_off, x.in_off)
    x = sc.expected(strs, sc.policies(len(strs), sc.HUFFMAN))
    for i, s in enumerate(strs):
        h = hpack_ref.huffman_encode(s)
        assert literal(x, i) == hpack_ref.encode_integer(len(h), 7, 0x80) + h
    assert literal(x, len(strs) - 2) == b"\x80"


def test_expected_decodes_back():
    strs, pol = sc.mixed_batch(600, 300, 20001)
    pol[pol == sc.VERBATIM] = sc.AUTO
    x = sc.expected(strs, pol)
    buf, at = x.flat.tobytes(), 0
    for i, s in enumerate(strs):
        got, used = hpack_ref.decode_string(buf[at:])
        assert got == s and used == x.out_len[i] and bool(buf[at] & 0x80) == bool(x.huff[i])
        at += used
    assert at == len(buf)


def test_rfc_c4_constants():
    strs = [b"www.example.com", b"no-cache", b"custom-key", b"custom-value"]
    x = sc.expected(strs)
    want = ["8cf1e3c2e5f23a6ba0ab90f4ff", "86a8eb10649cbf", "8825a849e95ba97d7f", "8925a849e95bb8e8b4bf"]
    assert [literal(x, i).hex() for i in range(4)] == want
    assert literal(sc.expected(strs, sc.policies(4, sc.RAW)), 0) == b"\x0f" + strs[0]


def test_decision_edge():
    strs, huff = sc.decision_edge()
    x = sc.expected(strs)
    assert np.array_equal(x.huff, huff) and huff.sum() == 4
    for i, s in enumerate(strs):
        n = len(s)
        bits = sum(hpack_ref.TABLE[b][1] for b in s)
        assert n in (3, 10, 127, 128) and bits == 8 * n + (-8, -7, 0, 1)[i % 4]
        assert x.out_len[i] == (n - 1 if huff[i] else n) + (1 if (n - 1 if huff[i] else n) < 127 else 2)
    assert sc.with_bits(10, 72).count(b"&") == 6 and sc.with_bits(10, 72).count(b"A") == 4
    # one byte alone is never shorter coded; neither are two 5-bit codes
    one = sc.expected([bytes((b,)) for b in range(256)])
    assert not one.huff.any() and (one.out_len == 2).all()
    two = sc.expected([bytes((a, b)) for a in ec.FIVE_BIT for b in ec.FIVE_BIT])
    assert not two.huff.any() and (two.out_len == 3).all()


def test_prefix_edges(geo):
    strs, pol, pay, huff = sc.prefix_edges_small()
    x = sc.expected(strs, pol)
    assert np.array_equal(x.huff, huff) and np.array_equal(x.out_len - x.plen, pay)
    want = {126: 1, 127: 2, 128: 2, 254: 2, 255: 3, 16510: 3, 16511: 4}
    assert [want[int(p)] for p in pay] == x.plen.tolist()
    # the Huffman payloads of 16510 and 16511 bytes come from more input than a tile holds: the one-lane path
    for i in np.nonzero(huff & (pay >= 16510))[0]:
        assert len(strs[i]) > geo.T
    for p, k in zip(sc.PREFIX_EDGES_RAW_ONLY, (4, 5)):
        assert len(hpack_ref.encode_integer(p, 7, 0)) == k
    # 2- and 3-octet prefixes only in the straddle batch
    s2, p2 = sc.prefix_straddle()
    x2 = sc.expected(s2, p2)
    assert len(s2) == 40 and set(x2.plen.tolist()) == {2, 3}


@pytest.mark.parametrize("plus", [0, 1])
@pytest.mark.parametrize("shift", [0, 5])
def test_in_cut(geo, plus, shift):
    strs, sh, _ = pc.in_cut(geo, plus, shift)
    plan, x = sc.plan_of(strs, None, sh, 0, geo)
    assert x.in_off[HEAD] + shift == geo.T + plus
    assert plan[0] == (0, HEAD - plus, "input") and len(plan) == 2 and plan[1][2] == "end"


@pytest.mark.parametrize("e", [1, 33])
def test_empties_on_cut(geo, e):
    strs = pc.empties_on_cut(geo, e)[0]
    plan, x = sc.plan_of(strs, None, 0, 0, geo)
    lens = np.diff(x.in_off)
    assert x.in_off[HEAD] == geo.T and (lens[HEAD : HEAD + e] == 0).all() and lens[HEAD + e] > 0
    assert (x.out_len[HEAD : HEAD + e] == 1).all()  # (an empty literal is the octet 00)
    assert plan[0] == (0, HEAD + e, "input")


def test_out_cut(geo):
    """30-bit codes under HUFFMAN: the representations pass the image within the tile's T input bytes; the same
    literals under AUTO are raw and the input binds"""
    per = geo.T // pc.OUT_CUT_N
    strs = pc.out_cut(geo, "thirty")[0]
    n = len(strs)
    plan, x = sc.plan_of(strs, sc.policies(n, sc.HUFFMAN), 0, 0, geo)
    rep = 30 * per // 8 + 3
    assert (x.out_len[: pc.OUT_CUT_N] == rep).all() and x.in_off[pc.OUT_CUT_N] == geo.T
    k = geo.I // rep
    assert 0 < k < pc.OUT_CUT_N and plan[0] == (0, k, "output") and plan[1][0] == k and plan[1][1] > 0
    plan, x = sc.plan_of(strs, None, 0, 0, geo)
    assert not x.huff.any() and plan[0] == (0, pc.OUT_CUT_N, "input")


def test_count_cut(geo):
    # Q empty or one-byte literals are at most Q input bytes and 2 Q bytes of representations: neither byte limit
    # binds, and a range of 3 Q of them is cut by count (encode_cases.count_cut gives every workgroup >= 3 Q)
    assert geo.Q + 16 <= geo.T and 2 * geo.Q + 16 <= geo.I
    m = 3 * geo.Q
    for per_in, per_out in ((0, 1), (1, 2)):
        io, oo = np.arange(m + 1) * per_in, np.arange(m + 1) * per_out
        for mis in (0, 15):
            assert ec.tile_plan(io, oo, mis, mis, geo) == [(0, geo.Q, "count"), (geo.Q, geo.Q, "count"),
                                                           (2 * geo.Q, geo.Q, "end")]


def test_lone_literals(geo):
    for nbytes in pc.lone_sizes(geo):
        for shift in (0, 1):
            strs = sc.lone(nbytes, shift)
            for pol in (sc.RAW, sc.AUTO, sc.VERBATIM):
                plan, x = sc.plan_of(strs, sc.policies(1, pol), shift, 0, geo)
                assert x.huff[0] == (pol == sc.AUTO)  # (header-like text: the Huffman form is shorter)
                # one tile only for T bytes at an aligned start, else no tile at all: the large-literal paths
                # (3 T + 5 raw bytes pass the image too)
                if (nbytes, shift) == (geo.T, 0):
                    assert plan == [(0, 1, "end")]
                else:
                    assert len(plan) == 1 and plan[0][:2] == (0, 0) and plan[0][2].startswith("input")


def test_multi_workgroup_batches(geo):
    x = sc.multi_wg_expected()
    assert len(x.out_len) == 20000 > 2 * geo.P and x.huff.mean() > 0.5
    u = sc.expected(sc.uniform_batch(20000, 300, 24000))
    assert u.huff.mean() < 0.1


def test_null_context_is_refused():
    from loona_amd import _lib

    L = _lib.lib()
    assert "hpk_encode_strings_packed" in _lib.EXPORTS and "hpk_string_len_batch" in _lib.EXPORTS
    assert (_lib.HPK_STR_AUTO, _lib.HPK_STR_RAW, _lib.HPK_STR_HUFFMAN, _lib.HPK_STR_VERBATIM) == (0, 1, 2, 3)
    b = (ctypes.c_uint8 * 64)()
    io = (ctypes.c_uint32 * 2)(0, 4)
    oo = (ctypes.c_uint32 * 2)()
    ol = (ctypes.c_uint32 * 1)()
    st = (ctypes.c_uint8 * 1)()
    for flags in (_lib.HPK_PTR_DEVICE, _lib.HPK_PTR_HOST, _lib.HPK_PTR_DEVICE | _lib.HPK_ASYNC):
        assert L.hpk_encode_strings_packed(None, b, 64, io, 1, None, b, 64, oo, ol, st, flags) == _lib.HPK_E_INVAL
        assert L.hpk_string_len_batch(None, b, 64, io, 1, None, ol, flags) == _lib.HPK_E_INVAL
    assert L.hpk_test_strings_geometry(None, None, None, None) == _lib.HPK_E_INVAL
