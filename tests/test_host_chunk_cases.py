"""The chunk cuts of the host-pointer batches, on the CPU (no GPU needed).

tests/emu/chunks_emu.cpp includes the REAL loona_amd/csrc/hpk_chunks.h and prints the chunk count and the cuts for
argument tuples. They are compared with the Python model of tests/host_chunk_cases.py on every placed case, on the
differential batch, on the edge tuples (n = 0, 1, 7, 8, 9; byte totals one below, on and one above 1, 2, 8 and 9
chunks' worth; no input bytes with 8 chunks' worth of output; both byte counts at HPK_MAX_OFFSET, which a 32-bit
product would wrap) and on seeded random batches, where the cuts must also be sound whatever the model says
(non-decreasing, cut[0] = 0, cut[chunks] = n). Every placed case is then shown to reach the edge it is named for,
on the model's cuts and on the oracle's answer. The replay is also built with -fsanitize=address,undefined and run
stand-alone on the same tuples (its offset array has exactly n + 1 entries, its cut array one poisoned entry per
slot: a read or a write past either is reported)."""

import os
import shutil
import subprocess

import numpy as np
import pytest

import host_chunk_cases as hc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CB, MC = hc.CHUNK_BYTES, hc.MAX_CHUNKS


def _build(d, name, flags):
    exe = str(d / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", *flags, "-I", os.path.join(REPO, "loona_amd", "csrc"),
                           os.path.join(HERE, "emu", "chunks_emu.cpp"), "-o", exe])
    return exe


def _run(exe, tuples):
    """tuples: ("count", in_bytes, out_bytes, n) or ("cuts", out_bytes, in_off) -> (process, consts, answers)"""
    lines = []
    for t in tuples:
        if t[0] == "count":
            lines.append("count %d %d %d" % t[1:])
        else:
            lines.append("cuts %d %d %s" % (t[1], len(t[2]) - 1, " ".join(str(int(x)) for x in t[2])))
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr
    assert "ok: %d tuples" % len(tuples) in p.stderr, p.stderr
    out = [[int(x) for x in line.split()[1:]] for line in p.stdout.splitlines()]
    assert len(out) == len(tuples) + 1
    return p, tuple(out[0]), out[1:]


def _model(t):
    if t[0] == "count":
        return [hc.chunk_count(*t[1:])]
    chunks, cut = hc.cuts_of(t[2], t[1])
    return [chunks] + cut


def _even(total, n):
    """in_off of n literals that share `total` bytes evenly"""
    return [total * i // n for i in range(n + 1)] if n else [total]


def edge_tuples():
    t = []
    for n in (0, 1, 7, 8, 9):
        t.append(("count", 1000, MC * CB, n))
        t.append(("cuts", MC * CB, _even(1000 if n else 0, n)))
    for k in (1, 2, 8, 9):
        for total in (k * CB - 1, k * CB, k * CB + 1):
            for in_bytes in (0, 1, total // 2, total - 1, total):
                t.append(("count", in_bytes, total - in_bytes, 20))
                t.append(("cuts", total - in_bytes, _even(in_bytes, 20)))
    t.append(("cuts", MC * CB, [0] * 21))  # no input bytes, 8 chunks' worth of output
    t.append(("cuts", MC * CB, [7] * 21))  # the same behind a base
    for n in (1, 7, 9, 1000):
        t.append(("count", hc.HPK_MAX_OFFSET, hc.HPK_MAX_OFFSET, n))
        t.append(("cuts", hc.HPK_MAX_OFFSET, _even(hc.HPK_MAX_OFFSET, n)))
    t.append(("cuts", hc.HPK_MAX_OFFSET, [0] * 9 + [hc.HPK_MAX_OFFSET]))  # every byte in the last literal
    t.append(("cuts", hc.HPK_MAX_OFFSET, [0] + [hc.HPK_MAX_OFFSET] * 9))  # and in the first
    return t


def random_tuples():
    rng = np.random.default_rng(4)
    t = []
    for _ in range(400):
        n = int(rng.integers(0, 40))
        lens = rng.integers(0, 50, n) * (rng.random(n) < 0.7)
        if n and rng.random() < 0.3:
            lens[int(rng.integers(0, n))] += int(rng.integers(0, 1 << 20))
        off = int(rng.integers(0, 9)) + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        t.append(("cuts", int(rng.integers(0, 10 * CB)), [int(x) for x in off]))
    return t


def case_tuples():
    t = [("cuts", int(hc.case(name).out_off[-1]), hc.case(name).in_off) for name in hc.CASE_NAMES]
    c, _ = hc.differential()
    return t + [("cuts", int(c.out_off[-1]), c.in_off)]


def all_tuples():
    return case_tuples() + edge_tuples() + random_tuples()


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host C++ compiler")
    return tmp_path_factory.mktemp("chunks_emu")


@pytest.fixture(scope="module")
def emu(workdir):
    return _build(workdir, "chunks_emu", [])


def check(tuples, consts, out):
    assert consts == (MC, CB)
    for t, got in zip(tuples, out):
        assert got == _model(t), t[:2]
        if t[0] == "cuts":  # and, whatever the model says, sound cuts
            n, chunks, cut = len(t[2]) - 1, got[0], got[1:]
            assert len(cut) == chunks + 1 and cut[0] == 0 and cut[-1] == n
            assert all(a <= b for a, b in zip(cut, cut[1:]))
            assert chunks <= MC and (chunks >= 1 or n == 0)


def test_model_equals_replay_on_every_case(emu):
    tuples = case_tuples()
    _, consts, out = _run(emu, tuples)
    check(tuples, consts, out)
    assert out[-1][0] == MC  # the differential batch is cut into 8 chunks


def test_model_equals_replay_on_edge_tuples(emu):
    tuples = edge_tuples()
    _, consts, out = _run(emu, tuples)
    check(tuples, consts, out)
    counts = {t[1:]: got[0] for t, got in zip(tuples, out) if t[0] == "count"}
    assert [counts[(1000, MC * CB, n)] for n in (0, 1, 7, 8, 9)] == [0, 1, 7, 8, 8]
    for k, want in ((1, (1, 1, 1)), (2, (1, 2, 2)), (8, (7, 8, 8)), (9, (8, 8, 8))):
        assert tuple(counts[(0, k * CB + d, 20)] for d in (-1, 0, 1)) == want
    assert counts[(hc.HPK_MAX_OFFSET, hc.HPK_MAX_OFFSET, 9)] == MC


def test_cuts_are_sound_for_any_input(emu):
    tuples = random_tuples()
    _, consts, out = _run(emu, tuples)
    check(tuples, consts, out)
    assert len({got[0] for got in out}) >= 5  # (the batches differ in their chunk counts)


def test_replay_under_host_sanitizers(workdir):
    """The same program with ASan and UBSan, stand-alone, on all the tuples."""
    tuples = all_tuples()
    exe = _build(workdir, "chunks_emu_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    p, consts, out = _run(exe, tuples)
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
    check(tuples, consts, out)


# ---- every case reaches the edge it is named for -----------------------------------------------------------------

def _cuts(name):
    c = hc.case(name)
    return (c,) + hc.cuts(c.in_off, c.out_off)


def test_case_list():
    assert len(hc.CASE_NAMES) == len(set(hc.CASE_NAMES)) and set(hc.DECODE_NAMES) | set(hc.ENCODE_NAMES) == set(hc.CASE_NAMES)
    for name in hc.CASE_NAMES:
        c = hc.case(name)
        n = len(c.lits)
        assert c.kind == ("encode" if name in hc.ENCODE_NAMES else "decode")
        assert n <= 80 and len(c.in_off) == len(c.out_off) == n + 1
        assert np.array_equal(np.diff(c.in_off), [len(x) for x in c.lits]) and (np.diff(c.out_off) >= 0).all()
        assert c.in_cap >= c.in_off[-1] and c.out_cap >= c.out_off[-1] and c.out_cap < 40 << 20
        chunks, _ = hc.cuts(c.in_off, c.out_off)
        assert chunks == {"small3": 1, "dense-long": 2}.get(name, min(MC, n)), name


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_collapsed(where):
    c, chunks, cut = _cuts(f"collapsed-{where}")
    big = c.meta["big"]
    assert len(c.lits[big]) * 8 > 7 * int(c.in_off[-1])
    assert cut[1:MC] == [big] * (MC - 1)  # chunks 1 .. 6 are empty
    assert (cut[1] - cut[0] > 0) == (where != "first") and cut[MC] - cut[MC - 1] == len(c.lits) - big
    ex = hc.expected_of(f"collapsed-{where}")
    assert not ex.status.any() and ex.out_len.all()


def test_no_input():
    c, chunks, cut = _cuts("no-input")
    assert c.in_off[-1] == 0 and chunks == MC and cut == [0] * MC + [20]
    ex = hc.expected_of("no-input")
    assert not ex.status.any() and not ex.out_len.any()


@pytest.mark.parametrize("n", [1, 3, 7])
def test_fewer_literals_than_chunks(n):
    c, chunks, cut = _cuts(f"few-{n}")
    assert chunks == n < MC and (int(c.in_off[-1]) + int(c.out_off[-1])) // CB >= MC


@pytest.mark.parametrize("how", ["on", "before", "after"])
def test_target_on_a_literals_end(how):
    c, chunks, cut = _cuts(f"target-{how}")
    tg = hc.targets(c)
    assert tg == [120 * j for j in range(1, MC)]
    for j in range(1, MC):
        end = int(c.in_off[3 * j])  # where literal 3 j - 1 ends
        assert end == tg[j - 1] + c.meta["d"]
        # one byte short of the target stays in the earlier chunk; on it (the tie) and past it open the later one
        assert cut[j] == (3 * j if how == "before" else 3 * j - 1)


def test_empty_literals_on_a_cut():
    c, chunks, cut = _cuts("empties-on-cut")
    tg, takers = hc.targets(c), c.meta["takers"]
    assert cut[1:MC] == takers[: MC - 1]
    for g, x in enumerate(takers):
        assert [len(c.lits[i]) for i in (x - 3, x - 2, x - 1, x + 1, x + 2, x + 3)] == [0] * 6 and len(c.lits[x]) > 0
        if g < MC - 1:
            assert int(c.in_off[x + 1]) - tg[g] == (1 if g % 2 == 0 else 0)


def test_cut_alignment():
    seen = []
    for shift in (0, 1, 15):
        c, chunks, cut = _cuts(f"align-{shift}")
        assert chunks == MC and [int(c.in_off[i]) % 16 for i in cut[1:MC]] == [shift] * (MC - 1)
        assert len(c.lits[0]) == shift
        seen.append((c.lits[1:], cut))
    assert seen[0] == seen[1] == seen[2]
    ex = [hc.expected_of(f"align-{shift}") for shift in (0, 1, 15)]
    assert all(np.array_equal(e.out_len[1:], ex[0].out_len[1:]) and not e.status.any() for e in ex)


@pytest.mark.parametrize("side", ["first", "last"])
@pytest.mark.parametrize("what", list(hc.ERRORS))
def test_errors_at_the_seams(what, side):
    name = f"seam-{what}-{side}"
    c, chunks, cut = _cuts(name)
    ex = hc.expected_of(name)
    rows = c.meta["rows"]
    assert chunks == MC and all(b > a for a, b in zip(cut, cut[1:]))
    assert rows == [cut[j] if side == "first" else cut[j + 1] - 1 for j in range(MC)]
    want = np.zeros(len(c.lits), np.uint8)
    want[rows] = hc.ERRORS[what]
    assert np.array_equal(ex.status, want)  # the neighbours across every cut are valid
    if what == "short":
        assert np.array_equal(ex.out_len[rows], np.diff(c.out_off)[rows]) and ex.out_len[rows].all()


@pytest.mark.parametrize("nbytes", hc.SEAM_SIZES)
def test_long_and_huge_at_the_seams(nbytes):
    name = f"seam-size-{nbytes}"
    c, chunks, cut = _cuts(name)
    k = c.meta["first_big"]
    assert len(c.lits[k]) == len(c.lits[k + 1]) == nbytes and chunks == MC
    at = [j for j in range(1, chunks) if cut[j] == k + 1]
    assert at and cut[at[0] - 1] <= k  # literal k is the last of a chunk, literal k + 1 the first of a later one
    ex = hc.expected_of(name)
    assert not ex.status.any() and ex.out_len[k + 1] == 8 * nbytes // 5


def test_dense_long_chunk_next_to_short():
    c, chunks, cut = _cuts("dense-long")
    assert chunks == 2 and cut == [0, 12, len(c.lits)]
    assert min(len(x) for x in c.lits[:12]) >= 64 and max(len(x) for x in c.lits[12:]) < 64


def test_exact_regions_across_cuts():
    c, chunks, cut = _cuts("exact-regions")
    ex = hc.expected_of("exact-regions")
    assert chunks == MC and not ex.status.any()
    assert np.array_equal(ex.out_len[:23], np.diff(c.out_off)[:23]) and (ex.out_len == 65).all()
    assert {int(c.out_off[i]) % 4 for i in cut[1:MC]} >= {1, 2, 3}  # region starts on a cut off the dword grid


def test_encode_cases():
    for name, short in (("encode-exact", False), ("encode-short", True)):
        c, chunks, cut = _cuts(name)
        ex = hc.expected_of(name)
        caps = np.diff(c.out_off)
        assert chunks == MC and np.array_equal(ex.out_len, np.minimum(caps, [hc.encoded_len(x) for x in c.lits]))
        rows = c.meta["rows"]
        assert rows == ([cut[3] - 1, cut[3], cut[5] - 1, cut[5]] if short else [])
        want = np.zeros(24, np.uint8)
        want[rows] = 4
        assert np.array_equal(ex.status, want)
        assert np.array_equal(ex.out_len[:23], caps[:23])
    assert not hc.expected_of("encode-text").status.any()


@pytest.mark.parametrize("kind", ["decode", "encode"])
def test_bases(kind):
    c, chunks, cut = _cuts(f"bases-{kind}")
    assert c.in_off[0] == 5 and c.out_off[0] == 7 and chunks == MC
    assert c.in_cap - c.in_off[-1] == 37 and c.out_cap - c.out_off[-1] == 37
    assert not hc.expected_of(f"bases-{kind}").status.any()


def test_differential_batch_has_every_status():
    c, ex = hc.differential()
    assert hc.cuts(c.in_off, c.out_off)[0] == MC and len(c.lits) == hc.DIFF_N
    assert all(int((ex.status == s).sum()) >= 10 for s in (1, 2, 3, 4)), np.bincount(ex.status)
    assert (ex.status == 0).sum() > 0.95 * hc.DIFF_N
