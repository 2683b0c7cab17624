"""The packed string-literal decode's cases (decode_strings_cases.py) on the CPU: expected() is
hpack_ref.decode_string window by window (with the C oracle's partial bytes where that raises a Huffman error),
and every placed case reaches the tile or window cut it claims, by the pack kernel's exported geometry
(hpk_test_pack_geometry)."""

import ctypes

import numpy as np
import pytest

import decode_strings_cases as dc
from hpk_util import hpack_ref, oracle_decode

KIND = {"TooManyOctets": dc.TOO_MANY, "NotEnoughOctets": dc.INT_SHORT}


@pytest.fixture(scope="module")
def geometry():
    from loona_amd import _lib

    t, l = ctypes.c_uint32(0), ctypes.c_uint32(0)
    assert _lib.lib().hpk_test_pack_geometry(ctypes.byref(t), ctypes.byref(l)) == _lib.HPK_E_OK
    assert t.value % 16 == 0 and t.value and l.value
    return t.value, l.value


def agrees(b, x):
    """x = expected(b) against hpack_ref.decode_string on every window"""
    raw = b.blob.tobytes()
    for i, (a, e) in enumerate(zip(b.str_off.tolist(), b.str_end.tolist())):
        got = x.flat[x.out_off[i] : x.out_off[i + 1]].tobytes()
        try:
            out, used = hpack_ref.decode_string(raw[a:e])
        except hpack_ref.DecoderError as err:
            if err.kind == "IntegerDecodingError":
                assert (x.status[i], x.consumed[i], got) == (KIND[err.detail], 0, b""), i
            elif err.detail == "NotEnoughOctets":
                assert (x.status[i], x.consumed[i], got) == (dc.STR_SHORT, 0, b""), i
            else:  # a Huffman error: status and partial bytes from the C oracle's decode of the payload
                assert err.detail[0] == "HuffmanDecoderError" and x.status[i] == err.detail[1], i
                ln, used = hpack_ref.decode_integer(raw[a:e], 7)
                st, part = oracle_decode(raw[a + used : a + used + ln])
                assert (st, part, used + ln) == (x.status[i], got, x.consumed[i]), i
            continue
        assert (x.status[i], got, x.consumed[i]) == (0, out, used), i


def test_expected_is_decode_string_on_prefix_shapes():
    shapes = dc.prefix_shapes()
    b = dc.batch_of([w for _, w in shapes])
    x = dc.expected(b)
    agrees(b, x)
    assert set(x.status.tolist()) >= {dc.OK, dc.TOO_MANY, dc.INT_SHORT, dc.STR_SHORT}
    # the same strings with windows to the blob's end: a cut integer now reads its neighbour's octets
    e = dc.to_end(b)
    agrees(e, dc.expected(e))


def test_expected_is_decode_string_on_batches(geometry):
    tile, lds = geometry
    vec = dc.error_vectors(200)
    assert {s for _, s in vec} == {1, 2, 3}
    for b in (dc.alternating(300), dc.empties_then_one(lds), dc.long_raw(tile), dc.mixed_batch(500, 36000)[0],
              dc.batch_of([dc.frame(p, True) for p, _ in vec])):
        x = dc.expected(b)
        agrees(b, x)
    assert np.array_equal(x.status, [s for _, s in vec]) and (x.consumed > 0).all()


def test_void_windows():
    b = dc.batch_of([dc.frame(b"abc", False), dc.frame(b"de", False), dc.frame(b"f", False)])
    off, end = b.str_off.copy(), b.str_end.copy()
    off[1], end[1] = end[1], off[1]  # str_off > str_end
    end[2] = b.blob.size + 1         # past in_cap
    x = dc.expected(dc.Batch(b.blob, off, end))
    assert x.status.tolist() == [0, dc.BAD_OFFSETS, dc.BAD_OFFSETS] and x.out_len.tolist() == [3, 0, 0]
    assert x.consumed.tolist() == [4, 0, 0] and x.flat.tobytes() == b"abc"


def test_round_trip_strings():
    strs = dc.round_trip_strings()
    assert len(strs) > 2000 and strs.count(b"") >= 20
    b = dc.batch_of([dc.frame_plain(s, i % 3 != 0) for i, s in enumerate(strs)])
    x = dc.expected(b)
    assert not x.status.any() and x.flat.tobytes() == b"".join(strs)
    assert np.array_equal(x.consumed, b.str_end - b.str_off)


def test_alternating_mixes_every_chunk():
    b = dc.alternating()
    x = dc.expected(b)
    assert not x.status.any() and (x.out_len >= 1).all() and (x.out_len <= 7).all()
    assert np.array_equal(x.huff, np.arange(len(x.huff)) % 2 == 1)
    total = int(x.out_off[-1])
    owner = np.repeat(x.huff, x.out_len)  # per output byte: its string's form
    for shift in (0, 1, 15):
        first = (-shift) % 16
        chunks = owner[first : first + (total - first) // 16 * 16].reshape(-1, 16)
        assert len(chunks) > 100 and (chunks.any(axis=1) & ~chunks.all(axis=1)).all()


def test_empties_pass_the_window(geometry):
    tile, lds = geometry
    x = dc.expected(dc.empties_then_one(lds))
    z = np.nonzero(x.out_len)[0]
    assert z[0] == 0 and z[1] - z[0] - 1 > lds and x.out_len[z[1]] == 12 and x.huff[z[1]]
    run = x.status[1 : z[1]]
    assert {0, dc.INT_SHORT, dc.STR_SHORT} == set(run.tolist())


def test_long_raw_covers_a_tile(geometry):
    tile, lds = geometry
    x = dc.expected(dc.long_raw(tile))
    i = int(np.argmax(x.out_len))
    assert x.out_len[i] == tile + 17 and not x.huff[i] and x.out_off[i] > 0 and x.out_off[i] % 16 != 0
    # whatever the destination's misalignment, one whole tile lies inside the string
    assert x.out_len[i] >= tile + 16


def test_sizes_batch():
    b = dc.sizes_batch()
    x = dc.expected(b)
    assert not x.status.any()
    assert {63, 64, 113, 65536} <= set(x.pay_len[x.huff].tolist())
    assert (~x.huff).any() and x.out_off[-1] > 8 * 65536 // 5
