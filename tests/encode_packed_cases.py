"""Cases for the packed encode (hpk_encode_batch_packed, hpk_encoded_len_batch), shared by
test_encode_packed_plan.py (CPU: a placed case reaches the cut it claims) and test_gpu_encode_packed.py (the
device result against the oracle, bit for bit).

A case is (strs, in_shift, out_shift): the plaintext literals and the misalignment of the input / output
blob's first byte from a 16-byte boundary. The packed encode's regions are the exact encodings back to back,
so a case's offsets are the exclusive sums of the plaintext lengths and of the oracle's encoded lengths:
expected() gives both with the oracle's bytes end to end. The kernel behind the packed form is hpk_encode2's
packed instantiation, which cuts its tiles by hpk_encode2's rule (encode_cases.tile_plan) on those exact
offsets; the length kernel walks the input in stretches of T bytes and carries a literal that passes a
stretch's end. Builders reuse encode_cases' where the shape is the same."""

import collections
import functools

import numpy as np

import encode_cases as ec
from hpk_util import oracle_encode_batch, pack

Expected = collections.namedtuple("Expected", "blob in_off out_off out_len flat")


def expected(strs):
    """The oracle's packed answer: out_len = its encoded lengths, out_off their exclusive sum, flat its valid
    bytes end to end. One oracle call."""
    blob, off = pack(strs)
    ob, oo, ol, st = oracle_encode_batch(blob, off)
    assert not st.any()
    ol = ol.astype(np.int64)
    eoff = np.zeros(len(strs) + 1, np.int64)
    np.cumsum(ol, out=eoff[1:])
    return Expected(blob, off.astype(np.int64), eoff, ol, ec.gather(ob, oo, ol))


LenGeo = collections.namedtuple("LenGeo", "S Q P")


@functools.lru_cache(maxsize=None)
def len_geometry():
    """the length pass's geometry (hpk_test_enclen_geometry): S = input bytes of a stretch, Q = literals it
    looks at per stretch, P = the literal count up to which a batch runs in one workgroup"""
    import ctypes

    from loona_amd import _lib

    v = [ctypes.c_uint32(0) for _ in range(3)]
    assert _lib.lib().hpk_test_enclen_geometry(*[ctypes.byref(x) for x in v]) == _lib.HPK_E_OK
    return LenGeo(*[x.value for x in v])


def len_plan(in_off, in_mis, lg):
    """How one workgroup of the length pass walks the literals [0, n): [(first, base, ended, carried)] per
    stretch, from the rule in the kernel's comments. A stretch covers the S input bytes from `base`, the
    16-byte boundary at or below `pos` (the first unfinished literal's start, or the previous stretch's end
    when that literal passed it); it looks at up to Q literals from `first`, `ended` of which end within
    the stretch; carried: the next literal started at or before the stretch's end and passes it, so its bits so
    far go on to the next stretch, which starts at base + S. Valid for good offsets and at most P literals."""
    io = np.asarray(in_off, np.int64) + in_mis
    n = len(io) - 1
    plan, cur = [], 0
    pos = int(io[0]) if n else 0
    while cur < n:
        base = pos & ~15
        cnt = min(lg.Q, n - cur)
        k = 0
        while k < cnt and int(io[cur + k + 1]) - base <= lg.S:
            k += 1
        carried = k < cnt
        plan.append((cur, base, k, carried))
        cur += k
        if carried:
            pos = base + lg.S
        elif cur < n:
            pos = int(io[cur])
    return plan


def lone(geo, nbytes, shift):
    rng = np.random.default_rng(11000 + nbytes % 1000 + shift)
    return [ec._text(rng, nbytes)], shift, 0


def lone_sizes(geo):
    return (geo.T, geo.T + 1, 3 * geo.T + 5)


def in_cut(geo, plus, shift):
    return ec.in_cut(geo, plus, shift)[0], shift, 0


def empties_on_cut(geo, e):
    return ec.in_cut(geo, 0, 0, e)[0], 0, 0


OUT_CUT_N, OUT_CUT_TAIL = 16, 8


def out_cut(geo, kind):
    """OUT_CUT_N literals of T / OUT_CUT_N bytes each (T input bytes in all: the input limit does not bind at
    an aligned start), then OUT_CUT_TAIL short ones. "thirty": 30-bit codes only, whose exact encodings pass
    the image within the tile's T input bytes; "five": 5-bit codes only; "alternate": the two byte by byte."""
    rng = np.random.default_rng(12000)
    per = geo.T // OUT_CUT_N
    a, b = np.frombuffer(ec.THIRTY_BIT, np.uint8), np.frombuffer(ec.FIVE_BIT, np.uint8)
    strs = []
    for n in [per] * OUT_CUT_N + list(rng.integers(1, 60, OUT_CUT_TAIL)):
        x, y = rng.choice(a, int(n)), rng.choice(b, int(n))
        if kind == "five":
            x = y
        elif kind == "alternate":
            x[1::2] = y[1::2]
        else:
            assert kind == "thirty"
        strs.append(x.astype(np.uint8).tobytes())
    return strs, 0, 0


def empties_between(geo):
    """Empty literals before, between and after non-empty ones, the non-empty ones ending on tile ends: the
    in-cut case with 2 empties on the cut, an empty literal first and three last."""
    s = ec.in_cut(geo, 0, 0, 2)[0]
    return [b""] + s + [b"", b"", b""], 0, 0


def count_cut(geo, cus, one_byte):
    return ec.count_cut(geo, cus, one_byte)[0], 0, 0


def text_batch(n, hi, seed, shifts=(0, 0)):
    rng = np.random.default_rng(seed)
    return [ec._text(rng, k) for k in rng.integers(0, hi + 1, n)], shifts[0], shifts[1]


@functools.lru_cache(maxsize=None)
def multi_wg():
    """20 000 text literals of 0..300 bytes: every tile and workgroup boundary is a shared 16-byte chunk"""
    return text_batch(20000, 300, 13000)


@functools.lru_cache(maxsize=None)
def multi_wg_expected():
    return expected(multi_wg()[0])
