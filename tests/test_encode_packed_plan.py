"""The packed encode's placed cases (encode_packed_cases.py) on the CPU: each case that claims a tile cut
reaches it. The packed form's encode kernel is hpk_encode2's packed instantiation, so its tiles are cut by
hpk_encode2's rule (encode_cases.tile_plan, geometry from hpk_test_encode_geometry), applied to the packed
form's own offsets: the exclusive sums of the plaintext lengths and of the oracle's encoded lengths. The
length kernel walks the input in stretches of T bytes from the 16-byte boundary at or below a literal's
start: a literal passes a stretch's end, and is carried, when its bytes end more than T past that boundary."""

import numpy as np
import pytest

import encode_cases as ec
import encode_packed_cases as pc
from encode_cases import HEAD, TAIL, tile_plan


@pytest.fixture(scope="module")
def geo():
    return ec.geometry()


def plan_of(case, geo):
    strs, in_shift, out_shift = case
    x = pc.expected(strs)
    assert len(strs) <= geo.P  # one workgroup: the model holds
    return tile_plan(x.in_off, x.out_off, in_shift & 15, out_shift & 15, geo), x


@pytest.mark.parametrize("plus", [0, 1])
@pytest.mark.parametrize("shift", [0, 5])
def test_in_cut(geo, plus, shift):
    plan, x = plan_of(pc.in_cut(geo, plus, shift), geo)
    assert x.in_off[HEAD] + shift == geo.T + plus
    assert plan[0] == (0, HEAD - plus, "input")  # ends at T: the tile's last literal; at T + 1: cut off
    assert len(plan) == 2 and plan[1][2] == "end"


@pytest.mark.parametrize("e", [1, 2, 33])
def test_empties_on_cut(geo, e):
    plan, x = plan_of(pc.empties_on_cut(geo, e), geo)
    lens = np.diff(x.in_off)
    assert x.in_off[HEAD] == geo.T and (lens[HEAD : HEAD + e] == 0).all() and lens[HEAD + e] > 0
    assert plan[0] == (0, HEAD + e, "input")


def test_empties_between(geo):
    plan, x = plan_of(pc.empties_between(geo), geo)
    lens = np.diff(x.in_off)
    assert lens[0] == 0 and (lens[-3:] == 0).all() and (lens[1 + HEAD : 3 + HEAD] == 0).all()
    assert x.in_off[1 + HEAD] == geo.T
    assert plan == [(0, 1 + HEAD + 2, "input"), (1 + HEAD + 2, TAIL + 3, "end")]  # tile 1 ends in empty literals


def test_lone_literals(geo):
    for nbytes in pc.lone_sizes(geo):
        for shift in (0, 1):
            plan, x = plan_of(pc.lone(geo, nbytes, shift), geo)
            assert x.in_off[-1] == nbytes
            # the encode: one tile only for T bytes at an aligned start, else no tile at all (the one-lane path)
            assert plan == ([(0, 1, "end")] if (nbytes, shift) == (geo.T, 0) else [(0, 0, "input")])


def test_len_plan_model():
    g = pc.LenGeo(S=64, Q=3, P=64)
    # whole literals within a stretch; the window's count; a restart at the next literal's 16-byte boundary
    assert pc.len_plan([0, 10, 20, 64], 0, g) == [(0, 0, 3, False)]
    assert pc.len_plan([0, 1, 2, 3, 40], 0, g) == [(0, 0, 3, False), (3, 0, 1, False)]
    assert pc.len_plan([0, 30, 70], 5, g) == [(0, 0, 1, True), (1, 64, 1, False)]
    # a literal that ends at the stretch's end ends in it; one byte more and it is carried
    assert pc.len_plan([0, 64], 0, g) == [(0, 0, 1, False)]
    assert pc.len_plan([0, 65], 0, g) == [(0, 0, 0, True), (0, 64, 1, False)]
    assert pc.len_plan([0, 64], 1, g) == [(0, 0, 0, True), (0, 64, 1, False)]
    # carried over several stretches, an empty literal at the end of the last
    assert pc.len_plan([0, 200, 200], 0, g) == [(0, 0, 0, True), (0, 64, 0, True), (0, 128, 0, True), (0, 192, 2, False)]
    # a literal that starts exactly at a stretch's end is carried with no bits
    assert pc.len_plan([0, 64, 70], 0, g) == [(0, 0, 1, True), (1, 64, 1, False)]


def test_lone_literals_length_carry(geo):
    """The length kernel's cross-tile carry, by a model of its walk with its own exported geometry: a lone
    literal of T bytes at an aligned start is one stretch with no carry; shifted by a byte, or of T + 1 bytes,
    it is carried once; 3 T + 5 bytes three times; 1 MiB (the GPU test's shift 3) through 64 stretches."""
    lg = pc.len_geometry()
    assert lg.S % 16 == 0 and lg.S and lg.Q and lg.P
    T = geo.T  # (the cases are built from the encode kernel's T: the claims below hold for the length pass's S)
    want = {(T, 0): 0, (T, 1): 1, (T + 1, 0): 1, (T + 1, 1): 1, (3 * T + 5, 0): 3, (3 * T + 5, 1): 3}
    for (nbytes, shift), carries in want.items():
        strs, sh, _ = pc.lone(geo, nbytes, shift)
        plan = pc.len_plan([0, len(strs[0])], sh & 15, lg)
        assert [p[3] for p in plan] == [True] * carries + [False], (nbytes, shift, plan)
        assert plan[-1][2] == 1 and all(p[2] == 0 for p in plan[:-1])
    plan = pc.len_plan([0, 1 << 20], 3, lg)
    assert len(plan) == (1 << 20) // lg.S + 1 and all(p[3] for p in plan[:-1]) and not plan[-1][3]
    # the in-cut cases: literal HEAD - 1 ends at the stretch's end (ends there) or one byte past it (carried)
    for plus in (0, 1):
        for shift in (0, 5):
            strs, sh, _ = pc.in_cut(geo, plus, shift)
            plan = pc.len_plan(pc.expected(strs).in_off, sh & 15, lg)
            assert plan[0] == (0, 0, HEAD - plus, True)


def test_count_cut(geo):
    # (encode_cases.count_cut's batches: test_encode_cases.py shows every workgroup gets >= 2 Q literals.) A
    # range of 3 Q empty or one-byte literals in exact regions is cut by count: the byte limits cannot bind
    assert geo.Q + 16 <= geo.T and 4 * geo.Q + 16 <= geo.I
    m = 3 * geo.Q
    for per_in, per_out in ((0, 0), (1, 1), (1, 4)):  # (a one-byte literal encodes to 1..4 bytes)
        io, oo = np.arange(m + 1) * per_in, np.arange(m + 1) * per_out
        for mis in (0, 15):
            assert tile_plan(io, oo, mis, mis, geo) == [(0, geo.Q, "count"), (geo.Q, geo.Q, "count"),
                                                        (2 * geo.Q, geo.Q, "end")]
    for one_byte in (False, True):
        strs = pc.count_cut(geo, 1, one_byte)[0]
        assert len(strs) == ec.count_cut_n(geo, 1) and all(len(s) == int(one_byte) for s in strs)


def test_out_cut(geo):
    per = geo.T // pc.OUT_CUT_N
    assert per * pc.OUT_CUT_N == geo.T and per % 4 == 0
    plan, x = plan_of(pc.out_cut(geo, "thirty"), geo)
    assert set(x.blob.tolist()) <= {10, 13, 22} and (x.out_len[: pc.OUT_CUT_N] == 30 * per // 8).all()
    assert x.in_off[pc.OUT_CUT_N] == geo.T and x.out_off[pc.OUT_CUT_N] == 30 * geo.T // 8 > geo.I
    k = geo.I // (30 * per // 8)  # whole literals within the image
    assert 0 < k < pc.OUT_CUT_N and plan[0] == (0, k, "output")  # the input limit did not bind: the output did
    assert plan[1][0] == k and plan[1][1] > 0
    plan, x = plan_of(pc.out_cut(geo, "five"), geo)
    assert set(x.blob.tolist()) <= set(ec.FIVE_BIT) and (x.out_len[: pc.OUT_CUT_N] == 5 * per // 8).all()
    assert plan[0] == (0, pc.OUT_CUT_N, "input")  # all T bytes, a sixth of the image
    plan, x = plan_of(pc.out_cut(geo, "alternate"), geo)
    assert (x.out_len[: pc.OUT_CUT_N] == 35 * (per // 2) // 8).all() and plan[0] == (0, pc.OUT_CUT_N, "input")


def test_multi_workgroup_batch(geo):
    strs = pc.multi_wg()[0]
    x = pc.multi_wg_expected()
    lens = np.diff(x.in_off)
    assert len(strs) == 20000 > 2 * geo.P and lens.min() == 0 and lens.max() == 300
    assert int(x.in_off[-1]) > 100 * geo.T and (np.diff(x.out_off) == x.out_len).all()
