"""The placed cases of decode_long_cases.py do what their names claim (no GPU needed), and the huge-literal
phase's replay (tests/emu/emu.cpp, the REAL per-piece functions of hpk_huge_piece.h under the workgroup's
protocol) decodes every huge one as the oracle does, under the 12-bit table of the workgroup-fill kernel and the
13-bit table of the wave kernel.

Where a code starts is established with the plain decoder decode_long_cases.walk (checked against the C oracle
here), never with the replay. From the replay's line per literal come the fix rounds, the pieces whose lead walk
ended, the terminal piece and its count.

Fix rounds. The truth moves one piece per round, so a stream that never resynchronises needs t - 1 rounds at least
to reach its terminal piece t (0-based): P - 2 for a literal walked to its end, which is what the clean and the
foreign-symbol endings are. A literal with EOS at 3/4 has t = 3 P / 4, and the pieces behind t are ignored, so its
bound is t - 1 (measured at P = 128: 94 to 125 rounds, at P = 1024: 766 to 1021). The stream of byte 10 with '0'
resynchronises inside the lead (0 rounds, whatever stands in front of it): asserted as that.

The replay is also built with -fsanitize=address,undefined and run stand-alone on the same case files: each literal's
input then ends with its last 16-byte chunk, so a chunk read past the clamp is a report."""

import os
import shutil
import subprocess

import numpy as np
import pytest

import decode_long_cases as dc
import san_util
from hpk_util import oracle_decode_batch, pack

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if not shutil.which("g++") or not shutil.which("gcc"):
        pytest.skip("no host C/C++ compiler")
    d = tmp_path_factory.mktemp("emu_long")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-D_GNU_SOURCE", "-c", os.path.join(REPO, "oracle", "hpk_oracle.c"),
                           "-o", str(d / "oracle.o")])
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(REPO, "loona_amd", "csrc"), "-I",
                           os.path.join(HERE, "emu"), os.path.join(HERE, "emu", "emu.cpp"), str(d / "oracle.o"), "-o",
                           str(d / "emu"), "-lpthread"])
    return str(d / "emu"), d


@pytest.fixture(scope="module")
def geo():
    g = dc.geometry("wave")
    assert g[:12] == dc.geometry("fill")[:12] and g.table == 4 and dc.geometry("fill").table == 2
    return g


def replay(emu, lits, tab, lanes, exe=None):
    """the replay's line per literal as a dict of ints (exe: another build of the program)"""
    d = emu[1]
    path = str(d / f"cases_{tab}.bin")
    dc.write_emu_file(path, lits)
    p = subprocess.run([exe or emu[0], "--file", path, str(lanes), str(tab)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "ok: 0 mismatches" in p.stdout, p.stdout[-3000:] + p.stderr
    if exe is not None:
        san_util.assert_no_reports(p)
    rows = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("lit ")]
    assert len(rows) == len(lits)
    return [dict(zip(r[2:-1:2], map(int, r[3:-1:2]))) for r in rows]


def test_case_names():
    """the list of cases and its count: no case is dropped"""
    want = {"noresync-": 8 * 2 * 3, "none-chain-": 2, "straddle30-d": 29, "straddle13-d": 12, "pair-on-boundary-": 4,
            "eos-at-": 5, "last-piece-": 12, "terminal-early": 1, "ov-pb": 2, "share-": 4, "huge-capacity-": 4,
            "long-sweep": 1, "long-ring": 1, "long-short-output": 1, "long-tail": 1, "long-claims-dense-": 9,
            "long-claims-sprinkled-": 9, "long-capacity-": 8, "neighbour-bytes-": 8}
    for prefix, k in want.items():
        assert len(dc.names(prefix)) == k, prefix
    assert len(dc.CASE_NAMES) == sum(want.values()) == 161 and len(set(dc.CASE_NAMES)) == 161
    for stream in ("len5", "len6", "len7", "len8", "len30", "cyc01", "cyc10_0"):  # these streams, each at both
        for tag in ("8k", "64k"):                                                  # sizes with the three endings
            for ending in ("clean", "foreign", "eos"):
                assert f"noresync-{stream}-{tag}-{ending}" in dc.CASE_NAMES
    assert [f"straddle30-d{d}" for d in range(1, 30)] == dc.names("straddle30-")
    assert [f"straddle13-d{d}" for d in range(1, 13)] == dc.names("straddle13-")
    assert dc.names("eos-at-") == ["eos-at-m30", "eos-at-m1", "eos-at-0", "eos-at-p1", "eos-at-last"]
    assert [int(n.rsplit("-", 1)[1]) for n in dc.names("long-claims-dense-")] == [63, 64, 65, 128, 129, 511, 512, 513, 1025]
    assert len(dc.HUGE_SINGLE) == 48 + 2 + 41 + 4 + 5 + 12 + 1 + 2


def test_geometry(geo):
    """the kernels' constants as the cases assume them, and the restated piece geometry at the sizes used"""
    assert (geo.block, geo.huge_min, geo.huge_max, geo.piece_min) == (1024, 8192, 16, 64)
    assert (geo.long_min, geo.long_big, geo.ring, geo.chunks, geo.steps, geo.claim, geo.waves, geo.obuf) == \
        (64, 1024, 32, 3, 8, 64, 8, 80)
    hg = lambda nb: dc.huge_geometry(nb, geo.block, geo.piece_min)  # noqa: E731
    assert hg(8192) == (128, 64, 256) and hg(65536) == (1024, 64, 256) and dc.sizes(geo) == (8192, 65536)
    assert hg(523264) == (1024, 511, 256) and hg(523265)[1:] == (512, 512) and hg(524288) == (1024, 512, 512)
    assert hg(8321) == (131, 64, 256) and [dc.last_piece_size(geo, k) for k in (1, 8, 9)] == [8321, 8328, 8329]
    assert dc.ring_lengths(geo)[:3] == [95, 96, 97] and dc.ring_lengths(geo)[-4:] == [127, 128, 129, 8191]
    assert len(dc.ring_lengths(geo)) == 37


@pytest.fixture(scope="module")
def walks():
    """the plain decoder's walk of every 8 KiB-class single-literal case (shared, never modified)"""
    return {n: dc.walk(dc.case(n).lits[0]) for n in dc.HUGE_SINGLE if len(dc.case(n).lits[0]) < 16384}


def test_walk_is_the_oracle(walks):
    """decode_long_cases.walk against the C oracle: status, length and bytes of every literal it is used on"""
    names = list(walks)
    blob, off = pack([dc.case(n).lits[0] for n in names])
    out, oo, ol, st = oracle_decode_batch(blob, off)
    for i, n in enumerate(names):
        w = walks[n]
        assert (w.status, len(w.syms)) == (int(st[i]), int(ol[i])), n
        assert bytes(w.syms) == out[int(oo[i]) : int(oo[i]) + int(ol[i])].tobytes(), n
        assert w.status == dc.case(n).meta["status"], n


@pytest.mark.parametrize("tab", [2, 4])
def test_huge_cases_replay(emu, geo, walks, tab):
    names = list(dc.HUGE_SINGLE)
    rows = dict(zip(names, replay(emu, [dc.case(n).lits[0] for n in names], tab, geo.block)))
    for n in names:
        r, c = rows[n], dc.case(n)
        assert r["status"] == c.meta["status"], n
        assert (r["P"], r["PB"]) == dc.huge_geometry(len(c.lits[0]), geo.block, geo.piece_min)[:2], n
    for n in dc.names("noresync-"):
        r, (_, stream, _, ending) = rows[n], n.split("-")
        if stream in dc.RESYNCS:
            assert r["rounds"] == 0, (n, r)
            continue
        if ending != "eos":
            assert r["term"] == r["P"] - 1, (n, r)
        else:
            assert abs(r["term"] - 3 * r["P"] // 4) <= 1, (n, r)
        assert r["rounds"] >= r["term"] - 1, (n, r)  # (P - 2 for the clean and the foreign endings)
    assert rows["noresync-len5-64k-clean"]["rounds"] == 1023
    assert rows["none-chain-1"]["none"] >= 1 and rows["none-chain-2"]["run"] >= 2
    for n in dc.names("last-piece-"):
        r, m = rows[n], dc.case(n).meta
        st_last = (r["P"] - 1) * r["PB"] * 8
        assert m["bytes"] - (r["P"] - 1) * r["PB"] == m["last"] == int(n.split("-")[2]), n
        assert r["term"] == r["P"] - 1, n
        assert r["c"] == sum(1 for p in walks[n].starts if p >= st_last), n  # the codes that start in the last piece
        if m["c0"]:
            assert r["c"] == 0, n
    assert rows["terminal-early"]["term"] == 1
    for n in dc.names("eos-at-"):
        assert rows[n]["term"] == dc.case(n).meta["bit"] // (rows[n]["PB"] * 8), n


def test_replay_of_the_batches_huge_literals(emu, geo):
    """the huge literals of the multi-literal cases too (both tables), and the smallest size with 64 lanes"""
    lits = []
    for n in dc.names("share-") + dc.names("huge-capacity-") + dc.names("neighbour-bytes-huge"):
        lits += [x for x in dc.case(n).lits if len(x) >= geo.huge_min]
    for tab in (2, 4):
        replay(emu, lits, tab, geo.block)
    replay(emu, [dc.case(n).lits[0] for n in dc.names("straddle30-")], 4, 64)


@pytest.fixture(scope="module")
def emu_san(emu):
    return san_util.build_emu(emu[1], "emu_san", san_util.ASAN, source="emu")


@pytest.mark.parametrize("tab", [2, 4])
def test_huge_cases_replay_under_host_sanitizers(emu, emu_san, geo, tab):
    """The same program with ASan and UBSan, stand-alone, on the case file of test_huge_cases_replay: every literal
    decodes as the oracle does (the program's own check), with the status and the piece geometry the case states."""
    names = list(dc.HUGE_SINGLE)
    rows = dict(zip(names, replay(emu, [dc.case(n).lits[0] for n in names], tab, geo.block, exe=emu_san)))
    for n in names:
        r, c = rows[n], dc.case(n)
        assert r["status"] == c.meta["status"], n
        assert (r["P"], r["PB"]) == dc.huge_geometry(len(c.lits[0]), geo.block, geo.piece_min)[:2], n
    assert rows["noresync-len5-64k-clean"]["rounds"] == 1023


def test_placed_codes(geo, walks):
    """straddle, pair, eos-at, terminal-early: the code starts at the stated bit relative to the boundary nx
    between pieces 1 and 2, by the plain decoder's walk"""
    nx = 2 * 64 * 8
    assert nx == dc._nx(geo)
    for bits, ds in ((30, range(1, 30)), (13, range(1, 13))):
        for d in ds:
            n = f"straddle{bits}-d{d}"
            w = walks[n]
            i = w.starts.index(nx - d)
            assert dc.LEN[w.syms[i]] == bits and w.starts[i + 1] == nx - d + bits > nx, n
    for n, l0, l1, rel in (("pair-on-boundary-55-m1", 5, 5, -1), ("pair-on-boundary-55-0", 5, 5, 0),
                           ("pair-on-boundary-55-p1", 5, 5, 1), ("pair-on-boundary-57-0", 5, 7, 0)):
        w = walks[n]
        i = w.starts.index(nx + rel)
        assert [dc.LEN[s] for s in w.syms[i - 2 : i + 1]] == [13, l0, l1], n  # a lookup starts at the first of the pair
        assert w.starts[i - 1] == nx + rel - l0, n
    for n, rel in (("eos-at-m30", -30), ("eos-at-m1", -1), ("eos-at-0", 0), ("eos-at-p1", 1)):
        assert walks[n].status == 3 and walks[n].end == nx + rel, n
    w = walks["eos-at-last"]
    assert w.status == 3 and w.end // (64 * 8) == 127
    w = walks["terminal-early"]
    assert w.status == 3 and 64 * 8 <= w.end < nx


def test_share_cases(geo):
    """the huge literals are workgroup 0's whole range, and their pieces fill the block as named"""
    for kind, total in (("exact", geo.block), ("plus1", geo.block + 128), ("full_then_small", geo.block + 128),
                        ("list_plus1", 17 * 128)):
        c = dc.case(f"share-{kind}")
        n, h = len(c.lits), c.meta["huge"]
        g = dc.blocks(n, sum(len(x) for x in c.lits), dc.CUS_MAX)
        assert dc.wg_range(n, g, 0) == (0, h) and g <= 8, kind
        assert all(len(x) >= geo.huge_min for x in c.lits[:h]) and all(len(x) == 1 for x in c.lits[h:]), kind
        assert sum(c.meta["P"]) == total, kind
    assert dc.case("share-list_plus1").meta["huge"] == geo.huge_max + 1
    assert dc.case("share-full_then_small").meta["P"] == [geo.block, 128]


def _oracle(name):
    x = dc.expected_of(name)
    return x, np.diff(x.in_off), x.in_off[:-1] % 16, x.out_off[:-1] % 16


def test_long_sweep_and_ring(geo):
    x, lens, ial, _ = _oracle("long-sweep")
    rows = dc.case("long-sweep").meta["rows"]
    assert len(rows) == (208 - geo.long_min + 1) * 16 * 4 == 9280
    idx = np.array([r[0] for r in rows])
    assert np.array_equal(lens[idx], [r[1] for r in rows]) and np.array_equal(ial[idx], [r[2] for r in rows])
    assert np.array_equal(x.out_len[idx], [r[3] for r in rows]) and not x.status.any()
    assert {(r[1], r[2]) for r in rows} == {(nb, al) for nb in range(geo.long_min, 209) for al in range(16)}
    five = idx[0::4]  # the 5-bit streams fill their decoded bound exactly
    assert np.array_equal(x.out_len[five], lens[five] * 8 // 5)
    assert set((x.out_off[:-1] % 16)[idx]) == set(range(16))  # back to back: every output alignment occurs
    x, lens, _, _ = _oracle("long-ring")
    rows = dc.case("long-ring").meta["rows"]
    assert [r[1] for r in rows[0::2]] == dc.ring_lengths(geo) and np.array_equal(lens, [r[1] for r in rows])
    assert np.array_equal(x.out_len, [r[3] for r in rows]) and not x.status.any()


def test_long_short_output_and_tail(geo):
    x, lens, _, oal = _oracle("long-short-output")
    rows = dc.case("long-short-output").meta["rows"]
    assert len(rows) == 6 * 16
    assert {(r[1], r[2]) for r in rows} == {(m, al) for m in (0, 1, 15, 16, 17) for al in range(16)}
    for i, m, al, st in rows:
        assert lens[i] >= geo.long_min and oal[i] == al and x.out_len[i] == m and x.status[i] == st, (i, m, al)
    x, lens, _, _ = _oracle("long-tail")
    rows = dc.case("long-tail").meta["rows"]
    assert (lens == dc.TAIL_BYTES).all() and dc.TAIL_BYTES >= geo.long_min
    assert [r[1] for r in rows] == [f"pad{p}" for p in range(8)] + [f"zero-in-pad{p}" for p in range(1, 8)] + \
        [f"cut{r}" for r in range(8, 30)] + [f"code{l}-ends" for l in (13, 14, 15, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 30)] + \
        ["eos-ends"]
    assert np.array_equal(x.status, [r[2] for r in rows])


@pytest.mark.parametrize("sprinkled", [False, True])
def test_long_claims(geo, sprinkled):
    """every workgroup's range holds `count` literals of the long phase, some of them listed at the front (>=
    long_big bytes); the dense batches' ranges are listed whole by the kernels' rule (more than half of the bytes
    of a range's first 2,048 literals in long literals), the sprinkled ones' are not"""
    for count in dc.CLAIM_COUNTS:
        c = dc.case(f"long-claims-{'sprinkled' if sprinkled else 'dense'}-{count}")
        lens = np.fromiter((len(x) for x in c.lits), np.int64, len(c.lits))
        n = len(lens)
        g = dc.blocks(n, int(lens.sum()), dc.CUS_MAX)
        assert g == (1 if c.meta["one_wg"] else dc.CUS_MAX), count
        if g > 1:  # the ranges between the first, the middle and the last one: one-byte literals
            assert (lens[slice(*dc.wg_range(n, g, 1))] == 1).all() and (lens[slice(*dc.wg_range(n, g, g - 2))] == 1).all()
        for w in sorted({0, g // 2, g - 1}):
            a, b = dc.wg_range(n, g, w)
            r = lens[a:b]
            assert n % g == 0 and len(r) == n // g
            assert ((r >= geo.long_min) & (r < geo.huge_min)).sum() == count, (count, w)
            assert (r >= geo.long_big).any() and (r < geo.long_big).any(), (count, w)
            head = r[:2048]
            assert (2 * head[head >= geo.long_min].sum() > head.sum()) == (not sprinkled), (count, w)
            if not sprinkled:
                assert len(r) == count


def test_capacity_and_neighbour_cases(geo):
    for nb, fam in ((geo.huge_min, "huge-capacity"), (200, "long-capacity-200"), (4000, "long-capacity-4000")):
        for which in dc.CAPACITIES:
            c = dc.case(f"{fam}-{which}")
            x = dc.expected_of(f"{fam}-{which}")
            dec, cap = c.meta["decoded"], c.meta["cap"]
            assert len(c.lits[1]) == nb and c.caps[1] == cap
            assert cap == {"bound": 8 * nb // 5, "exact": dec, "minus1": dec - 1, "7": 7}[which]
            assert (x.status[1], x.out_len[1]) == ((0, dec) if cap >= dec else (4, cap)), (fam, which)
            assert x.status[0] == 0 and x.status[2] == 0
    for which in dc.NEIGHBOURS:
        for mod in (1, 15):
            c = dc.case(f"neighbour-bytes-{which}-{mod}")
            assert sum(len(x) for x in c.lits) % 16 == mod and len(c.lits) == 2
            assert len(c.lits[1]) == (200 if which.startswith("long") else geo.huge_min)
            assert dc.expected_of(f"neighbour-bytes-{which}-{mod}").status[1] == c.meta["status"]
