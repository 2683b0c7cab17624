"""The placed cases of the small-call mode's persistent kernel (persist_cases.py) contain what their names say, by the
module's models of the kernel's dispatch, store plan and literal distribution (no GPU needed). The models themselves
are checked against hpk_persist_lit.h by the replay (test_persist_emulation.py: the program restates the same
dispatch test and store plan and runs the real functions)."""

import itertools

import numpy as np
import pytest

import persist_cases as pc
from decode_long_cases import bound, walk


@pytest.fixture(scope="module")
def geo():
    return pc.geometry()


def lit_of(b, i):
    return b.blob[int(b.in_off[i]) : int(b.in_off[i + 1])].tobytes()


def test_geometry_is_the_kernels(geo):
    assert geo == (113, 8, 48, 256)
    assert geo.slot_max + 15 <= 16 * geo.slot_chunks  # staged at every misalignment
    assert bound(geo.slot_max) + 3 + 4 + 1 <= 4 * geo.out_dwords


def test_names():
    want = set(pc.GOOD_NAMES) | set(pc.BAD_NAMES) | {"over_max"} | {f"counts-{n}" for n in (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4096)}
    assert set(pc.names()) == want
    for name in pc.names():
        b = pc.batch(name)
        assert len(b.in_off) - 1 <= pc.SM_MAX + 1 and len(b.in_off) == len(b.out_off)


def test_gaps_are_empty_literals(geo):
    for name in ("store_plan", "in_place", "short_regions", "global"):
        b = pc.batch(name)
        v = pc.verdicts(geo, b)
        gaps = [i for i, x in enumerate(v) if x == "empty"]
        rows = {r[0] for r in b.meta["rows"]}
        assert gaps and not rows & set(gaps)
        for i in rows:  # a canary gap in front of every placed literal
            assert v[i - 1] == "empty" and b.out_off[i] - b.out_off[i - 1] >= 1, (name, i)


def test_store_plan(geo):
    b = pc.batch("store_plan")
    v = pc.verdicts(geo, b)
    rows = b.meta["rows"]
    assert {(r, c) for _, r, c in rows} == set(itertools.product(range(16), pc.STORE_COUNTS)) and len(rows) == 16 * 26
    assert bound(geo.slot_max) == max(pc.STORE_COUNTS)  # the top count is the longest staged literal's bound
    pieces = np.zeros(5, np.int64)
    for i, res, count in rows:
        assert v[i] == "staged_bound" and b.out_off[i] % 16 == res
        w = walk(lit_of(b, i))
        assert len(w.syms) == count and w.status == (0 if count else 1)
        p = pc.store_plan(int(b.out_off[i]), count)
        assert p.head + 4 * p.lead + 16 * p.groups + 4 * p.trail + p.tail == count
        assert p.head == min((-res) % 4, count) and p.head < 4 and p.tail < 4 and p.lead < 4 and p.trail < 4
        pieces += np.asarray(p) > 0
    assert (pieces > 0).all()
    # every arm of the plan by itself: each head and tail size, 1-3 leading and trailing dwords, 0 and the most groups
    plans = [pc.store_plan(int(b.out_off[i]), c) for i, _, c in rows]
    for k in range(4):
        assert any(p.head == k for p in plans) and any(p.tail == k for p in plans)
        assert any(p.lead == k for p in plans) and any(p.trail == k for p in plans)
    assert max(p.groups for p in plans) == 180 // 16 and any(p.groups == 0 and p.lead + p.trail for p in plans)


def test_in_place(geo):
    b = pc.batch("in_place")
    v = pc.verdicts(geo, b)
    rows = b.meta["rows"]
    assert {(r, n) for _, r, n in rows} == set(itertools.product(range(16), pc.IN_LENGTHS))
    chunks = set()
    for i, res, nb in rows:
        assert v[i] == "staged_bound" and b.in_off[i] % 16 == res and b.in_off[i + 1] - b.in_off[i] == nb
        assert walk(lit_of(b, i)).status == 0
        chunks.add(((int(b.in_off[i + 1]) + 15) >> 4) - (int(b.in_off[i]) >> 4))
    assert {1, 2, geo.slot_chunks - 1, geo.slot_chunks} <= chunks and max(chunks) == geo.slot_chunks
    assert any(r == 15 and nb == geo.slot_max and b.in_off[i + 1] % 16 == 0 for i, r, nb in rows)
    assert geo.slot_max in pc.IN_LENGTHS  # (at residue 15 it ends with its eighth chunk's last byte)


def test_short_regions(geo):
    b = pc.batch("short_regions")
    v = pc.verdicts(geo, b)
    x = pc.expected_of("short_regions")
    kinds, after = set(), 0
    for i, count, cap, st, want, which in b.meta["rows"]:
        assert v[i] == "staged_bytes" and b.out_off[i + 1] - b.out_off[i] == cap < bound(len(lit_of(b, i)))
        assert (x.status[i], x.out_len[i]) == (want, min(count, cap)), (i, which)
        kinds.add((which, st))
        after += st != 0 and cap <= count
    assert kinds == set(itertools.product(("zero", "minus1", "count", "between", "bound_minus1"), (0, 1, 2, 3)))
    assert after >= 3 * 8  # literals whose error comes after the capacity is reached


def test_global(geo):
    b = pc.batch("global")
    v = pc.verdicts(geo, b)
    x = pc.expected_of("global")
    rows = b.meta["rows"]
    assert {(nb, r, w) for _, nb, r, w, _, _ in rows} == set(itertools.product(pc.GLOBAL_LENGTHS, range(8), pc.GLOBAL_CAPS))
    assert len({int(b.in_off[i]) % 16 for i, *_ in rows}) == 16
    for i, nb, res, which, count, want in rows:
        assert v[i] == "global" and b.out_off[i] % 8 == res and b.in_off[i + 1] - b.in_off[i] == nb
        cap = int(b.out_off[i + 1] - b.out_off[i])
        assert cap == {"bound": bound(nb), "count": count, "minus1": count - 1, "minus2": count - 2, "zero": 0}[which]
        assert (x.status[i], x.out_len[i]) == (want, min(count, cap))
    assert {3, 0, 4} <= set(x.status[[r[0] for r in rows]].tolist())


def test_mixed_wave(geo):
    b = pc.batch("mixed_wave")
    v = pc.verdicts(geo, b)
    n = len(v)
    assert n == 2 * geo.threads and "bad" not in v
    for wave in range(n // 64):
        lanes = v[64 * wave : 64 * wave + 64]
        assert set(zip(lanes, lanes[1:])) == set(itertools.product(pc.VERDICTS, repeat=2)), wave
    assert {pc.owner(geo, i, pc.SM_WGS)[0] for i in range(n)} == {0, 1}
    x = pc.expected_of("mixed_wave")
    for verdict in ("staged_bound", "staged_bytes", "global"):
        got = {int(x.status[i]) for i in range(n) if v[i] == verdict}
        assert {0, 1} <= got, (verdict, got)  # the error mix reaches each way
    assert {0, 1, 2, 3} <= {int(x.status[i]) for i in range(n) if v[i] == "staged_bound"}
    assert 4 in {int(x.status[i]) for i in range(n) if v[i] == "staged_bytes"}


def test_counts_and_distribution(geo):
    G, t = pc.SM_WGS, geo.threads
    assert pc.count_list(geo, G, pc.SM_MAX) == [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4096]
    assert pc.count_list(geo, 1, 4096)[-4:] == [255, 256, 257, 4096] and 16 * t + 1 in pc.count_list(geo, 16, 8192)
    for n in pc.count_list(geo, G, pc.SM_MAX):
        b = pc.batch(f"counts-{n}")
        assert len(b.in_off) - 1 == n and "bad" not in pc.verdicts(geo, b)
        own = [pc.owner(geo, i, G) for i in range(n)]
        assert len(set(own)) == n  # one lane and round per literal
        per = [sum(1 for w, _, _ in own if w == g) for g in range(G)]
        assert per == [sum(min(t, max(0, n - (r * G + g) * t)) for r in range(n // (G * t) + 1)) for g in range(G)]
    assert pc.owner(geo, G * t, G) == (0, 0, 1) and pc.owner(geo, G * t - 1, G) == (G - 1, t - 1, 0)
    assert pc.owner(geo, pc.SM_MAX - 1, G)[2] == pc.SM_MAX // (G * t) - 1
    assert len(pc.batch("over_max").in_off) - 1 == pc.SM_MAX + 1


def test_bad(geo):
    seen = set()
    for name in pc.BAD_NAMES:
        b = pc.batch(name)
        i, n = b.meta["literal"], len(b.in_off) - 1
        io, oo = b.in_off, b.out_off
        assert pc.fault(int(io[i]), int(io[i + 1]), int(oo[i]), int(oo[i + 1]), b.in_cap, b.out_cap) == b.meta["fault"], name
        assert pc.verdicts(geo, b)[i] == "bad"
        assert b.blob.size == b.in_cap == int(pc.counts_batch(n).in_off[-1]) + pc.IN_SLACK
        seen.add((b.meta["fault"], "first" if i == 0 else "last" if i == n - 1 else "wg1"))
        if 0 < i < n - 1:
            assert pc.owner(geo, i, pc.SM_WGS)[0] == 1
        # whatever the offsets say, the kernel's tests keep every access of a literal it decodes inside the blobs
        for k, verdict in enumerate(pc.verdicts(geo, b)):
            if verdict != "bad":
                assert 0 <= io[k] <= io[k + 1] <= b.in_cap and 0 <= oo[k] <= oo[k + 1] <= b.out_cap
    assert seen == set(itertools.product(pc.FAULTS, ("first", "last", "wg1")))
