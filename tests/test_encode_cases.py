"""The encode edge cases (encode_cases.py) on the CPU: every case does what its name claims, by the
tile-plan model of the kernel's cuts (a placed test must not silently miss its edge), and the library's CPU
batch path (hpk_encode_batch_cpu) matches the oracle on every one of them, the short capacities included
(status 4, out_len == cap, the encoding's first cap bytes)."""

import numpy as np
import pytest

import encode_cases as ec
from encode_cases import HEAD, TAIL, tile_plan

from loona_amd import _lib

GUARD = 4096
FILL = 0xAB


@pytest.fixture(scope="module")
def geo():
    return ec.geometry()


def test_geometry_export(geo):
    import ctypes

    assert geo.T % (64 * geo.B) == 0  # whole waves of threads, B bytes each
    assert geo.T % 16 == 0 and geo.I % 16 == 0 and geo.T and geo.I and geo.Q and geo.B and geo.P
    assert geo.B == 32  # one start-map word per thread (the builders' thread edges assume a u32 of bytes)
    v = [ctypes.c_uint32(0) for _ in range(5)]
    for miss in range(5):  # any NULL pointer is refused
        args = [None if i == miss else ctypes.byref(x) for i, x in enumerate(v)]
        assert _lib.lib().hpk_test_encode_geometry(*args) == _lib.HPK_E_INVAL


def test_tile_plan_model():
    g = ec.Geo(T=64, I=48, Q=3, B=4, P=64)
    # by count, then by input at == T, with the base rounded down
    assert tile_plan([0, 1, 2, 3, 4, 64, 65], [0] * 7, 0, 0, g) == [(0, 3, "count"), (3, 2, "input"), (5, 1, "end")]
    assert tile_plan([0, 64], [0, 0], 0, 0, g) == [(0, 1, "end")]
    assert tile_plan([0, 64], [0, 0], 1, 0, g) == [(0, 0, "input")]
    assert tile_plan([16, 80], [0, 0], 1, 0, g) == [(0, 0, "input")]
    assert tile_plan([17, 80], [0, 0], 15, 0, g) == [(0, 1, "end")]  # starts at 32, ends at 95: 63 bytes from 32
    # by output, == I fits and + 1 does not; both limits at once
    assert tile_plan([0, 1, 2], [0, 48, 50], 0, 0, g) == [(0, 1, "output"), (1, 1, "end")]
    assert tile_plan([0, 1, 2], [0, 48, 50], 0, 1, g) == [(0, 0, "output"), (1, 1, "end")]
    assert tile_plan([0, 70], [0, 50], 0, 0, g) == [(0, 0, "input+output")]
    # empty literals on a cut stay with the tile they end
    assert tile_plan([0, 64, 64, 64, 70], [0] * 5, 0, 0, g) == [(0, 3, "count"), (3, 1, "end")]
    assert tile_plan([0, 64, 64, 70], [0] * 4, 0, 0, g) == [(0, 2, "input"), (2, 1, "end")]


def plan_of(case, geo):
    _, io, oo = ec.layout(case)
    return tile_plan(io, oo, case[2] & 15, case[3] & 15, geo), io, oo


@pytest.mark.parametrize("plus", [0, 1])
@pytest.mark.parametrize("shift", [0, 5])
def test_in_cut_placed(geo, plus, shift):
    c = ec.case(f"in_cut_{'plus1' if plus else 'eq'}-in{shift}")
    plan, io, oo = plan_of(c, geo)
    assert len(c[0]) <= geo.P and c[2] == shift
    assert io[HEAD] + shift == geo.T + plus  # (base16 == 0: the blob starts `shift` bytes into a chunk)
    assert plan[0] == (0, HEAD - plus, "input")  # == T: literal HEAD - 1 is tile 0's last; + 1: it is cut off
    assert (np.diff(oo) == ec.expected(c).want_len).all()  # exact regions


@pytest.mark.parametrize("plus", [0, 1])
@pytest.mark.parametrize("shift", [0, 7])
def test_out_cut_placed(geo, plus, shift):
    full = ec.out_cut(geo, plus, shift)
    k = full[4]
    c = ec.case(f"out_cut_{'plus1' if plus else 'eq'}-out{shift}")
    assert c[0] == full[0]
    plan, io, oo = plan_of(c, geo)
    assert len(c[0]) <= geo.P and c[3] == shift
    assert oo[k] + shift == geo.I + plus
    assert plan[0] == (0, k - plus, "output")
    assert (np.diff(oo) == ec.bound(np.diff(io))).all()  # bound regions


def test_lone_T_placed(geo):
    c = ec.case("lone_T-aligned")
    assert len(c[0][0]) == geo.T and plan_of(c, geo)[0] == [(0, 1, "end")]
    c = ec.case("lone_T-shift1")
    assert len(c[0][0]) == geo.T and plan_of(c, geo)[0] == [(0, 0, "input")]
    c = ec.case("lone_T-T_plus1")
    assert len(c[0][0]) == geo.T + 1 and plan_of(c, geo)[0] == [(0, 0, "input")]
    c = ec.case("lone_T-big_region")
    assert len(c[0][0]) == 10 and c[1][0] == geo.I + 16 and plan_of(c, geo)[0] == [(0, 0, "output")]


@pytest.mark.parametrize("pos", [0, 20, 39])
def test_serial_positions_placed(geo, pos):
    c = ec.case(f"serial_positions-{pos}")
    plan, _, _ = plan_of(c, geo)
    assert len(c[0]) == 40 and len(c[0][pos]) == 2 * geo.T
    at = [i for i, p in enumerate(plan) if p[1] == 0]
    assert len(at) == 1 and plan[at[0]][0] == pos
    # the first, a middle and the last step of the workgroup's range
    assert (at[0] == 0) == (pos == 0) and (at[0] == len(plan) - 1) == (pos == 39)


def test_empty_tiles_placed(geo):
    for sh in (0, 5):
        c = ec.case(f"empty_tiles-64-out{sh}")
        plan, io, oo = plan_of(c, geo)
        assert plan == [(0, 64, "end")] and io[-1] == 0 and oo[-1] == 0 and c[3] == sh
    # the count-cut batches: every workgroup of a grid of at most 2 CUs gets at least 2 Q literals
    n = ec.count_cut_n(geo, ec.CUS_MAX)
    assert n // (2 * ec.CUS_MAX) >= 2 * geo.Q
    for cus in (1, 64, 256, 304):
        assert ec.count_cut_n(geo, cus) // (2 * cus) >= 2 * geo.Q
    # and a workgroup's range of such literals is cut by count: neither byte limit can bind
    assert geo.Q + 16 <= geo.T and 4 * geo.Q + 16 <= geo.I
    m = 3 * geo.Q
    for per_in, per_out in ((0, 0), (1, 4)):
        io, oo = np.arange(m + 1) * per_in, np.arange(m + 1) * per_out
        for mis in (0, 15):
            assert tile_plan(io, oo, mis, mis, geo) == [(0, geo.Q, "count"), (geo.Q, geo.Q, "count"),
                                                        (2 * geo.Q, geo.Q, "end")]
    c = ec.case("empty_tiles-count_cut_one_byte", 1)
    assert len(c[0]) == ec.count_cut_n(geo, 1) and all(len(s) == 1 for s in c[0]) and (c[1] == 4).all()
    c = ec.case("empty_tiles-count_cut_empty", 1)
    assert len(c[0]) == ec.count_cut_n(geo, 1) and not any(c[0]) and not c[1].any()


@pytest.mark.parametrize("e", [1, 2, 33])
def test_empties_on_cut_placed(geo, e):
    c = ec.case(f"empties_on_cut-{e}")
    plan, io, _ = plan_of(c, geo)
    lens = np.diff(io)
    assert len(c[0]) == HEAD + e + TAIL <= geo.P
    assert io[HEAD] == geo.T and (lens[HEAD : HEAD + e] == 0).all() and lens[HEAD - 1] > 0 and lens[HEAD + e] > 0
    assert plan[0] == (0, HEAD + e, "input")  # the empty literals end at T too: they close tile 0


def test_thread_edges_placed(geo):
    ps = ec.thread_edge_ps(geo)
    W = 64 * geo.B
    assert ps[: 2 * geo.B + 1] == list(range(2 * geo.B + 1)) and ps[-3:] == [W - 1, W, W + 1]
    for p in ps:
        for e in (0, 1, 3):
            c = ec.thread_edges(geo, p, e)
            plan, io, oo = plan_of(c, geo)
            lens = np.diff(io)
            assert plan == [(0, len(lens), "end")] and len(lens) <= geo.P
            assert list(lens[: 6 + e]) == [p] + [0] * e + [1, geo.B - 1, geo.B, geo.B + 1, 3 * geo.B]
            run = lens[6 + e :]
            assert (run == 1).sum() == 40 and (run == 0).sum() == 8 and (run[5::6] == 0).all()
            assert (np.diff(oo) == ec.bound(lens)).all()


def test_tight_cases_placed(geo):
    c = ec.case("tight_deep")
    x = ec.expected(c)
    lens, caps = np.diff(x.in_off), np.diff(x.out_off)
    W = 64 * geo.B
    assert len(lens) <= geo.P and {1500, 2 * W + 3, 40} <= set(lens.tolist())
    kinds = set()
    for n, cap, w in zip(lens.tolist(), caps.tolist(), x.want_len.tolist()):
        kinds.add((n, "exact" if cap == w else "zero" if cap == 0 else "one" if cap == 1 else "half" if cap == w // 2
                   else "minus1" if cap == w - 1 else "bound" if cap == ec.bound(n) else "?"))
    assert len(kinds) == 30 and not any(k == "?" for _, k in kinds)
    assert (x.status == 4).sum() == 20 and (x.status == 0).sum() == 10
    # a literal whose later threads start past the image, counted from its region's start
    c = ec.case("tight_deep-past_image")
    plan, io, oo = plan_of(c, geo)
    assert plan == [(0, 3, "end")]
    assert oo[1] * 8 + 30 * (io[2] - io[1] - geo.B) > 8 * (geo.I + 256) and oo[2] - oo[1] == 100
    for pos in (0, 15, 29):
        c = ec.case(f"one_tight_in_safe_tile-{pos}")
        plan, io, oo = plan_of(c, geo)
        assert plan == [(0, 30, "end")]
        tight = np.nonzero(np.diff(oo) * 8 < 30 * np.diff(io))[0]
        assert list(tight) == [pos]  # the one literal that flips the tile to the checked pass 2
        assert not ec.expected(c).status.any()


def test_all_exact_and_code_extremes_placed(geo):
    x = ec.expected_of("all_exact-in3-out13")
    lens = np.diff(x.in_off)
    assert len(lens) == 20000 and lens.max() == 200 and 0.08 < (lens == 0).mean() < 0.13
    assert (np.diff(x.out_off) == x.want_len).all() and not x.status.any()
    assert ec.case("all_exact-in3-out13")[2:] == (3, 13) and ec.case("all_exact-in0-out0")[2:] == (0, 0)
    x = ec.expected_of("code_extremes-thirty")
    lens = np.diff(x.in_off)
    assert len(lens) == 2000 and lens.max() == 70 and lens.min() == 0
    assert (x.want_len == ec.bound(lens)).all() and (np.diff(x.out_off) == x.want_len).all()  # no slack at all
    assert set(x.blob.tolist()) == {10, 13, 22}
    x = ec.expected_of("code_extremes-five")
    assert (x.want_len == (5 * np.diff(x.in_off) + 7) // 8).all() and set(x.blob.tolist()) == set(ec.FIVE_BIT)
    x = ec.expected_of("code_extremes-alternate")
    assert (x.want_len == (30 * ((lens + 1) // 2) + 5 * (lens // 2) + 7) // 8).all()


def check_cpu(name, case, x):
    """hpk_encode_batch_cpu on a case, in guard | shift | regions | guard buffers, against the oracle's answer x"""
    _, _, in_shift, out_shift = case
    n = len(x.in_off) - 1
    src = np.zeros(in_shift + x.blob.size + 1, np.uint8)
    src[in_shift : in_shift + x.blob.size] = x.blob
    total = int(x.out_off[-1])
    big = np.full(GUARD + out_shift + total + GUARD, FILL, np.uint8)
    out = big[GUARD + out_shift :]
    ol = np.full(max(n, 1), 7, np.uint32)
    st = np.full(max(n, 1), 9, np.uint8)
    io, oo = x.in_off.astype(np.uint32), x.out_off.astype(np.uint32)
    rc = _lib.lib().hpk_encode_batch_cpu(src[in_shift:].ctypes.data, io.ctypes.data, n, out.ctypes.data, oo.ctypes.data,
                                         ol.ctypes.data, st.ctypes.data, 4)
    assert rc == _lib.HPK_E_OK, name
    assert np.array_equal(st[:n], x.status), name
    assert np.array_equal(ol[:n].astype(np.int64), x.out_len), name
    assert np.array_equal(ec.gather(out, x.out_off, x.out_len), x.flat), name
    assert (big[: GUARD + out_shift] == FILL).all() and (out[total:] == FILL).all(), name


@pytest.mark.parametrize("name", ec.CASE_NAMES)
def test_cpu_batch_matches_oracle(name):
    cus = 2 if "count_cut" in name else ec.CUS_MAX  # (the count does not matter to the CPU path: a smaller batch)
    check_cpu(name, ec.case(name, cus), ec.expected_of(name, cus))


def test_cpu_batch_matches_oracle_thread_edges(geo):
    for p in ec.thread_edge_ps(geo):
        for e in (0, 1, 3):
            c = ec.thread_edges(geo, p, e)
            check_cpu(f"thread_edges p={p} e={e}", c, ec.expected(c))
