"""Placed edge cases for the encode tile kernel (hpk_encode2), shared by test_encode_cases.py (CPU: the
cases do what their names claim, the CPU batch path matches the oracle on them) and test_gpu_encode.py
(the kernel against the oracle, bit for bit).

The cases are placed relative to the kernel's own geometry (hpk_test_encode_geometry): T = input bytes
per tile, I = bytes of the LDS output image, Q = literals per tile, B = input bytes per thread (W = 64 B,
a wave's bytes), P = the literal count up to which a batch runs in one workgroup. tile_plan() restates
how a workgroup cuts its range into tiles, from the rule in the kernel's comments: the tests use it to
prove that a case reaches the edge it was built for.

A case is (strs, out_cap_per_literal, in_shift, out_shift): the literals, each literal's output region
size, and the misalignment of the input / output blob's first byte from a 16-byte boundary. "Bound" is
a region of ceil(30 len / 8) bytes, "exact" the true encoded length. layout() and expected() turn a case
into offsets and the oracle's answer (status 0, or 4 with the encoding's first `cap` bytes)."""

import collections
import ctypes
import functools

import numpy as np

from hpk_util import oracle_encode_batch, pack

Geo = collections.namedtuple("Geo", "T I Q B P")
CUS_MAX = 256  # a safe upper figure for the CUs of one device (the count-cut batches scale with it)

FIVE_BIT = b"012aceiost"  # the ten 5-bit codes (RFC 7541 App. B)
THIRTY_BIT = bytes([10, 13, 22])  # the three 30-bit byte codes
TEXT_MAX_BITS = 19  # the longest code of 0x20..0x7E ('\\')

_BYTE = [bytes((i,)) for i in range(256)]


@functools.lru_cache(maxsize=None)
def geometry():
    from loona_amd import _lib

    v = [ctypes.c_uint32(0) for _ in range(5)]
    assert _lib.lib().hpk_test_encode_geometry(*[ctypes.byref(x) for x in v]) == _lib.HPK_E_OK
    return Geo(*[x.value for x in v])


def bound(n):
    return (30 * np.asarray(n, np.int64) + 7) // 8


def tile_plan(in_off, out_off, in_mis, out_mis, geo):
    """How one workgroup cuts the literals [0, n) into tiles: [(first, count, cut_reason)].

    From the current literal `first`, whose input starts at gin = in_off[first] + in_mis and whose region
    starts at gout = out_off[first] + out_mis, a tile takes the longest prefix of literals that ends, in
    input, within T bytes of gin rounded down to 16, and, in output, within I bytes of gout rounded down
    to 16, and that has at most Q literals. cut_reason says what kept the next literal out: "input",
    "output", "input+output", "count", or "end" (no literal left). count == 0: the literal `first` fits
    no tile and goes to the one-lane path alone. Valid for batches of at most P literals."""
    io = np.asarray(in_off, np.int64) + in_mis
    oo = np.asarray(out_off, np.int64) + out_mis
    n = len(io) - 1
    plan = []
    cur = 0
    while cur < n:
        b16, ob16 = int(io[cur]) & ~15, int(oo[cur]) & ~15
        c, why = 0, "end"
        while cur + c < n:
            if c == geo.Q:
                why = "count"
                break
            fin = int(io[cur + c + 1]) - b16 <= geo.T
            fout = int(oo[cur + c + 1]) - ob16 <= geo.I
            if not (fin and fout):
                why = "input+output" if not (fin or fout) else "output" if fin else "input"
                break
            c += 1
        plan.append((cur, c, why))
        cur += max(c, 1)
    return plan


def layout(case):
    """(blob u8, in_off i64 [n+1], out_off i64 [n+1]) of a case."""
    strs, caps, _, _ = case
    blob, off = pack(strs)
    oo = np.zeros(len(strs) + 1, np.int64)
    np.cumsum(np.asarray(caps, np.int64), out=oo[1:])
    return blob, off.astype(np.int64), oo


def gather(buf, starts, lens):
    """buf[starts[i] : starts[i] + lens[i]] laid end to end"""
    lens = np.asarray(lens, np.int64)
    tot = int(lens.sum())
    if tot == 0:
        return np.zeros(0, np.uint8)
    ends = np.cumsum(lens)
    idx = np.repeat(np.asarray(starts, np.int64)[: len(lens)] - (ends - lens), lens) + np.arange(tot)
    return buf[idx]


def _lens_of(strs):
    return np.fromiter((len(s) for s in strs), np.int64, len(strs))


def _exact(strs):
    """the true encoded length of every literal (one oracle call)"""
    blob, off = pack(strs)
    return oracle_encode_batch(blob, off)[2].astype(np.int64)


def _text(rng, n):
    return rng.integers(0x20, 0x7F, int(n), dtype=np.uint8).tobytes()


def _rand(rng, n):
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


def _parts(rng, total, k, lo):
    """k lengths >= lo that sum to total"""
    assert total >= k * lo
    cuts = np.sort(rng.integers(0, total - k * lo + 1, k - 1))
    return (np.diff(np.concatenate([[0], cuts, [total - k * lo]])) + lo).astype(np.int64)


# ---- the builders -----------------------------------------------------------------------------

HEAD = 10  # the literals that make up tile 0 in the cut cases
TAIL = 10  # short literals after them


def in_cut(geo, plus, in_shift, empties=0):
    """Text literals with exact regions (19 bits per byte at most: the image limit does not bind);
    literal HEAD - 1 ends at i1 - base16 == T + plus, then `empties` empty literals, then TAIL short ones."""
    rng = np.random.default_rng(1000 + 10 * plus + in_shift + 100 * empties)
    lens = list(_parts(rng, geo.T + plus - in_shift, HEAD, 200)) + [0] * empties + list(rng.integers(1, 300, TAIL))
    strs = [_text(rng, n) for n in lens]
    return strs, _exact(strs), in_shift, 0


def out_cut(geo, plus, out_shift):
    """Bound regions; literal k - 1's region ends at o1 - ob16 == I + plus (k = the returned case's
    out_cut_index), then TAIL short literals. The regions' sum is hit with literals of 4 m bytes (bound
    15 m) and up to 14 one-byte literals (bound 4 each)."""
    rng = np.random.default_rng(2000 + 10 * plus + out_shift)
    need = geo.I + plus - out_shift
    ones = (4 * need) % 15  # 4 * ones = need (mod 15)
    assert (need - 4 * ones) % 15 == 0 and need > 4 * ones
    m = _parts(rng, (need - 4 * ones) // 15, 12, 20)
    lens = [4 * int(x) for x in m[:6]] + [1] * ones + [4 * int(x) for x in m[6:]]
    k = len(lens)
    assert int(bound(lens).sum()) == need
    lens += list(rng.integers(1, 200, TAIL))
    strs = [_rand(rng, n) for n in lens]
    return strs, bound(lens), 0, out_shift, k


def lone_T(geo, kind):
    rng = np.random.default_rng(3000)
    if kind in ("aligned", "shift1"):  # exactly T bytes: a tile at an aligned start, one lane otherwise
        strs = [_text(rng, geo.T)]
        return strs, _exact(strs), 0 if kind == "aligned" else 1, 0
    if kind == "T_plus1":
        strs = [_text(rng, geo.T + 1)]
        return strs, _exact(strs), 0, 0
    assert kind == "big_region"  # a tiny literal whose region is larger than the image
    return [_rand(rng, 10)], np.array([geo.I + 16], np.int64), 0, 0


def serial_positions(geo, pos):
    """A literal of 2 T bytes (one lane) as literal `pos` of 40 otherwise short ones, bound regions."""
    rng = np.random.default_rng(4000 + pos)
    lens = rng.integers(0, 120, 40)
    lens[pos] = 2 * geo.T
    strs = [_rand(rng, n) for n in lens]
    return strs, bound(lens), 3, 5


def empty_tiles_small(geo, out_shift):
    return [b""] * 64, np.zeros(64, np.int64), 0, out_shift


def count_cut_n(geo, cus):
    return 3 * geo.Q * (2 * cus) + 1


def count_cut(geo, cus, one_byte):
    """3 Q (2 CUs) + 1 literals, empty or of one byte with bound regions: the grid is at most 2 CUs
    workgroups and the ranges are balanced by bytes + 16 per literal, equal for equal literals, so every
    workgroup gets at least 3 Q literals and cuts its first two tiles at Q literals (neither byte limit
    can bind: Q literals are at most Q input bytes and 4 Q bytes of regions)."""
    n = count_cut_n(geo, cus)
    if not one_byte:
        return [b""] * n, np.zeros(n, np.int64), 0, 0
    rng = np.random.default_rng(5000)
    strs = [_BYTE[b] for b in rng.integers(0, 256, n, dtype=np.uint8).tolist()]
    return strs, np.full(n, 4, np.int64), 0, 0


def thread_edges(geo, p, e):
    """Bound regions: a literal of p bytes, e empty ones, then literals around a thread's B bytes, then 40
    one-byte literals with an empty one after every fifth."""
    rng = np.random.default_rng(6000 + 7 * p + e)
    B = geo.B
    lens = [p] + [0] * e + [1, B - 1, B, B + 1, 3 * B]
    for i in range(40):
        lens.append(1)
        if i % 5 == 4:
            lens.append(0)
    strs = [_rand(rng, n) for n in lens]
    return strs, bound(lens), 0, 0


def thread_edge_ps(geo):
    W = 64 * geo.B
    return list(range(0, 2 * geo.B + 1)) + [W - 1, W, W + 1]


def tight_deep(geo):
    """Capacities far below the encoding: 30 literals of 1500, 2 W + 3, 40, 7 and 200 bytes, each length
    with each of: exact, 0, 1, half the encoding, the encoding - 1, bound."""
    rng = np.random.default_rng(7000)
    W = 64 * geo.B
    lens = [(1500, 2 * W + 3, 40, 7, 200)[i % 5] for i in range(30)]
    strs = [_rand(rng, n) for n in lens]
    ex = _exact(strs)
    caps = [(int(x), 0, 1, int(x) // 2, int(x) - 1, int(bound(n)))[i % 6] for i, (x, n) in enumerate(zip(ex, lens))]
    return strs, np.asarray(caps, np.int64), 0, 0


def tight_past_image(geo):
    """One literal of T bytes of 30-bit codes with 100 bytes of room (its later threads' bit positions,
    counted from the region's start, lie past the image), between two ordinary literals."""
    rng = np.random.default_rng(7100)
    strs = [_rand(rng, 33), bytes(rng.choice(list(THIRTY_BIT), geo.T - 64).astype(np.uint8)), _rand(rng, 20)]
    return strs, np.array([int(bound(33)), 100, int(bound(20))], np.int64), 0, 0


def one_tight_in_safe_tile(geo, pos):
    """30 literals in one tile, bound regions, except literal `pos`: exact (the tile's pass 2 is the
    checked one for every literal)."""
    rng = np.random.default_rng(8000 + pos)
    lens = rng.integers(0, 300, 30)
    lens[pos] = 150
    strs = [_rand(rng, n) for n in lens]
    caps = bound(lens)
    caps[pos] = _exact([strs[pos]])[0]
    return strs, caps, 0, 0


def all_exact(geo, in_shift, out_shift):
    """20 000 literals of 0..200 bytes, 10 % empty, every region exact: back to back, so every tile end
    chunk and every workgroup boundary is shared with a neighbour's live bytes."""
    rng = np.random.default_rng(9000)
    lens = rng.integers(0, 201, 20000)
    lens[rng.random(20000) < 0.1] = 0
    strs = [_rand(rng, n) for n in lens]
    return strs, _exact(strs), in_shift, out_shift


def code_extremes(geo, kind):
    """2 000 literals of 0..70 bytes of 30-bit codes only, 5-bit codes only, or the two alternating byte
    by byte; bound regions (which the 30-bit literals fill to the last byte)."""
    rng = np.random.default_rng(9500)
    lens = rng.integers(0, 71, 2000)
    a, b = np.frombuffer(THIRTY_BIT, np.uint8), np.frombuffer(FIVE_BIT, np.uint8)
    strs = []
    for n in lens:
        x, y = rng.choice(a, int(n)), rng.choice(b, int(n))
        if kind == "five":
            x = y
        elif kind == "alternate":
            x[1::2] = y[1::2]
        else:
            assert kind == "thirty"
        strs.append(x.astype(np.uint8).tobytes())
    return strs, bound(lens), 0, 0


# ---- the cases by name (what both test files parametrise over) -----------------------------------

def _case_table(geo, cus):
    t = {}
    for plus in (0, 1):
        for sh in (0, 5):
            t[f"in_cut_{'plus1' if plus else 'eq'}-in{sh}"] = lambda plus=plus, sh=sh: in_cut(geo, plus, sh)
        for sh in (0, 7):
            t[f"out_cut_{'plus1' if plus else 'eq'}-out{sh}"] = lambda plus=plus, sh=sh: out_cut(geo, plus, sh)[:4]
    for k in ("aligned", "shift1", "T_plus1", "big_region"):
        t[f"lone_T-{k}"] = lambda k=k: lone_T(geo, k)
    for pos in (0, 20, 39):
        t[f"serial_positions-{pos}"] = lambda pos=pos: serial_positions(geo, pos)
    for sh in (0, 5):
        t[f"empty_tiles-64-out{sh}"] = lambda sh=sh: empty_tiles_small(geo, sh)
    t["empty_tiles-count_cut_empty"] = lambda: count_cut(geo, cus, False)
    t["empty_tiles-count_cut_one_byte"] = lambda: count_cut(geo, cus, True)
    for e in (1, 2, 33):
        t[f"empties_on_cut-{e}"] = lambda e=e: in_cut(geo, 0, 0, e)
    t["tight_deep"] = lambda: tight_deep(geo)
    t["tight_deep-past_image"] = lambda: tight_past_image(geo)
    for pos in (0, 15, 29):
        t[f"one_tight_in_safe_tile-{pos}"] = lambda pos=pos: one_tight_in_safe_tile(geo, pos)
    t["all_exact-in0-out0"] = lambda: all_exact(geo, 0, 0)
    t["all_exact-in3-out13"] = lambda: all_exact(geo, 3, 13)
    for k in ("thirty", "five", "alternate"):
        t[f"code_extremes-{k}"] = lambda k=k: code_extremes(geo, k)
    return t


# (thread_edges is a sweep of 3 (2 B + 4) small calls: the tests loop over thread_edge_ps x (0, 1, 3))
CASE_NAMES = tuple(_case_table(None, 0))  # (the names do not depend on the geometry)


@functools.lru_cache(maxsize=4)
def case(name, cus=CUS_MAX):
    """The named case. `cus` matters to the count-cut batches only."""
    return _case_table(geometry(), cus)[name]()


Expected = collections.namedtuple("Expected", "blob in_off out_off want_len out_len status flat")


def expected(case_):
    """The oracle's answer to a case: want_len = the true encoded lengths, out_len = min(want_len, cap),
    status = 4 where the encoding is longer than the region, flat = every literal's first out_len encoded
    bytes, end to end. One oracle call."""
    blob, io, oo = layout(case_)
    ob, ooo, want, st = oracle_encode_batch(blob, io.astype(np.uint32))
    assert not st.any()
    want = want.astype(np.int64)
    caps = np.diff(oo)
    ol = np.minimum(want, caps)
    status = np.where(want > caps, 4, 0).astype(np.uint8)
    return Expected(blob, io, oo, want, ol, status, gather(ob, ooo, ol))


@functools.lru_cache(maxsize=2)
def expected_of(name, cus=CUS_MAX):
    return expected(case(name, cus))
