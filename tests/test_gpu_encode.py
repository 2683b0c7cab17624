"""The encode tile kernel (hpk_encode2) at its placed edges, against the C oracle bit for bit: no tolerance.

The cases come from encode_cases.py, which places them relative to the kernel's own geometry
(hpk_test_encode_geometry); test_encode_cases.py proves, with a model of the tile cuts, that each case
reaches the edge it is named for. One checker serves every test: the output is guard | regions | guard,
everything prefilled, out_len and status prefilled with values the kernel never writes; afterwards every
literal has the oracle's status (0, or 4 when its region is shorter than its encoding), out_len ==
min(encoded length, capacity), the encoding's first out_len bytes in its region, and no byte outside the
regions has changed. Bytes of a region past out_len are unspecified (hpk.h) and not looked at."""

import time

import numpy as np
import pytest

import encode_cases as ec
from encode_cases import HEAD, tile_plan
from hpk_util import oracle_encode

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 4096
SLACK = 64  # bytes of out_blob past the last region: not to be written either
FILL = 0xAB
BAD_N, BAD_J = 20000, 12345


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU)")
    from loona_amd import HuffmanCodec

    c = HuffmanCodec(0, stream=torch.cuda.current_stream())
    yield c
    c.close()


@pytest.fixture(scope="module")
def geo():
    return ec.geometry()


@pytest.fixture(scope="module")
def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def off_dev(a):
    return to_dev(np.asarray(a, np.int64).astype(np.uint32).view(np.int32))


class Buffers:
    """The device buffers of one call: the input at `in_shift` bytes past a 16-byte boundary, the output
    blob at `out_shift` past one between two guards, out_len prefilled 7, status prefilled 9."""

    def __init__(self, blob, n, total, in_shift, out_shift, slack=SLACK):
        src = np.zeros(in_shift + blob.size + 1, np.uint8)
        src[in_shift : in_shift + blob.size] = blob
        self.src = to_dev(src)[in_shift:]
        self.lead = GUARD + out_shift
        self.total = total
        self.big = torch.full((self.lead + total + slack + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.out = self.big[self.lead : self.lead + total + slack]
        self.ol = torch.full((max(n, 1),), 7, dtype=torch.int32, device="cuda")
        self.st = torch.full((max(n, 1),), 9, dtype=torch.uint8, device="cuda")
        self.n = n

    def results(self):
        big = self.big.cpu().numpy()
        return big, big[self.lead :], self.ol.cpu().numpy()[: self.n].astype(np.int64), self.st.cpu().numpy()[: self.n]

    def assert_outside_untouched(self, big, what):
        assert (big[: self.lead] == FILL).all(), f"{what}: bytes before the first region changed"
        assert (big[self.lead + self.total :] == FILL).all(), f"{what}: bytes at or past the last region's end changed"


def check_case(codec, case, x, what):
    """Encode the case on the device and compare with the oracle's answer x (encode_cases.expected)."""
    n = len(x.in_off) - 1
    b = Buffers(x.blob, n, int(x.out_off[-1]), case[2], case[3])
    dio, doo = off_dev(x.in_off), off_dev(x.out_off)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    codec.encode_into(b.src, dio, b.out, doo, b.ol, b.st, device=True, sync=True)
    dt = time.perf_counter() - t0
    big, out, ol, st = b.results()
    bad = np.nonzero(st != x.status)[0]
    assert bad.size == 0, f"{what}: status differs at {bad[:10]}: {st[bad[:10]]} for {x.status[bad[:10]]}"
    bad = np.nonzero(ol != x.out_len)[0]
    assert bad.size == 0, f"{what}: out_len differs at {bad[:10]}: {ol[bad[:10]]} for {x.out_len[bad[:10]]}"
    got = ec.gather(out, x.out_off, x.out_len)
    if not np.array_equal(got, x.flat):
        first = int(np.nonzero(got != x.flat)[0][0])
        lit = int(np.searchsorted(np.cumsum(x.out_len), first, side="right"))
        raise AssertionError(f"{what}: encoded bytes differ, first in literal {lit} (input bytes "
                             f"{x.in_off[lit]}..{x.in_off[lit + 1]}, region {x.out_off[lit]}..{x.out_off[lit + 1]})")
    b.assert_outside_untouched(big, what)
    return dt


def run_named(codec, name, cus=ec.CUS_MAX):
    dt = check_case(codec, ec.case(name, cus), ec.expected_of(name, cus), name)
    print(f"\n{name}: {len(ec.case(name, cus)[0])} literals, encode call {dt * 1e3:.3f} ms")


def names(prefix):
    return [n for n in ec.CASE_NAMES if n.startswith(prefix)]


@pytest.mark.parametrize("name", names("in_cut_"))
def test_in_cut(codec, name):
    run_named(codec, name)


@pytest.mark.parametrize("name", names("out_cut_"))
def test_out_cut(codec, name):
    run_named(codec, name)


@pytest.mark.parametrize("name", names("lone_T-"))
def test_lone_T(codec, name):
    run_named(codec, name)


@pytest.mark.parametrize("name", names("serial_positions-"))
def test_serial_positions(codec, name):
    run_named(codec, name)


@pytest.mark.parametrize("name", names("empty_tiles-"))
def test_empty_tiles(codec, cus, name):
    run_named(codec, name, cus)


@pytest.mark.parametrize("name", names("empties_on_cut-"))
def test_empties_on_cut(codec, name):
    run_named(codec, name)


def test_thread_edges(codec, geo):
    total = 0.0
    for p in ec.thread_edge_ps(geo):
        for e in (0, 1, 3):
            c = ec.thread_edges(geo, p, e)
            total += check_case(codec, c, ec.expected(c), f"thread_edges p={p} e={e}")
    print(f"\nthread_edges: {3 * len(ec.thread_edge_ps(geo))} calls, encode calls {total * 1e3:.3f} ms in all")


@pytest.mark.parametrize("name", names("tight_deep"))
def test_tight_deep(codec, name):
    run_named(codec, name)


@pytest.mark.parametrize("name", names("one_tight_in_safe_tile-"))
def test_one_tight_in_safe_tile(codec, name):
    run_named(codec, name)


@pytest.mark.parametrize("name", names("all_exact-"))
def test_all_exact(codec, name):
    run_named(codec, name)


@pytest.mark.parametrize("name", names("code_extremes-"))
def test_code_extremes(codec, name):
    run_named(codec, name)


# ---- bad offsets ----------------------------------------------------------------------------------

_bad_base = None


def bad_base():
    """20 000 short text literals with bound regions; literal BAD_J - 1 has 60 bytes and BAD_J 5, so that
    literal BAD_J - 1 stretched over both (what a decreasing in_off[BAD_J] makes of it) still fits its region."""
    global _bad_base
    if _bad_base is None:
        rng = np.random.default_rng(77)
        lens = rng.integers(0, 61, BAD_N)
        lens[BAD_J - 1], lens[BAD_J] = 60, 5
        text = rng.integers(0x20, 0x7F, int(lens.sum()), dtype=np.uint8)
        cuts = np.concatenate([[0], np.cumsum(lens)])
        strs = [text[cuts[i] : cuts[i + 1]].tobytes() for i in range(BAD_N)]
        case = (strs, ec.bound(lens), 0, 0)
        _bad_base = (case, ec.expected(case))
    return _bad_base


def check_prefix_good(x, out, ol, st, upto, what, skip=()):
    """literals [0, upto) are status 0 with the oracle's bytes (but for `skip`)"""
    keep = np.ones(upto, bool)
    keep[list(skip)] = False
    idx = np.nonzero(keep)[0]
    assert (st[:upto] == 0).all(), f"{what}: a literal before the first bad one is not status 0: {np.nonzero(st[:upto])[0][:10]}"
    assert np.array_equal(ol[idx], x.want_len[idx]), what
    fl = np.concatenate([[0], np.cumsum(x.out_len)])
    assert np.array_equal(ec.gather(out, x.out_off[idx], x.want_len[idx]), ec.gather(x.flat, fl[idx], x.want_len[idx])), what


@pytest.mark.parametrize("kind", ["in_decreasing", "out_decreasing", "past_in_cap", "past_out_cap", "huge"])
def test_encode_bad_offsets(codec, kind):
    """hpk.h's device-pointer contract on the encode side: a literal whose offsets decrease or pass a
    capacity gets HPK_BAD_OFFSETS and out_len 0, as do the literals of its workgroup's range after it; every
    other literal is encoded as usual; the synchronous call raises, the asynchronous one leaves the sticky
    flag for check(); nothing outside the regions is written; the same buffers then encode normally.
    (The inputs are never placed so that a read outside the blob would fault: the kernel's reads are
    clamped to the blob by construction, which is argued from its code, not provoked.)"""
    from loona_amd import _lib

    BAD = _lib.HPK_BAD_OFFSETS
    case, x = bad_base()
    n, j = BAD_N, BAD_J
    io, oo = x.in_off.copy(), x.out_off.copy()
    first_bad, skip = j, ()
    if kind == "in_decreasing":
        io[j] = io[j + 1] + 3  # (literal j - 1 becomes a longer, valid literal: checked on its own below)
        skip = (j - 1,)
    elif kind == "out_decreasing":
        oo[j] = oo[j + 1] + 3  # (literal j - 1 only gains capacity)
    elif kind == "past_in_cap":
        io[j + 1 :] += 1 << 20
    elif kind == "past_out_cap":
        oo[-1] += 64
        first_bad = n - 1
    else:
        io[j] = 0xFFFFFFF0
        oo[j] = 0xFFFFFFF0
        first_bad = j - 1
    b = Buffers(x.blob, n, int(x.out_off[-1]), 0, 0, slack=0)  # (out_cap == the regions' end)
    dio, doo = off_dev(io), off_dev(oo)
    with pytest.raises(RuntimeError, match="hpk_encode_batch"):
        codec.encode_into(b.src, dio, b.out, doo, b.ol, b.st, device=True, sync=True)
    big, out, ol, st = b.results()
    assert set(np.unique(st)) <= {0, BAD} and st[first_bad] == BAD
    assert (ol[st == BAD] == 0).all()
    # the literals before the first bad one are all encoded, and the bad ones are one run from it on (the
    # rest of its workgroup's range; with offsets past the input's capacity, the rest of the batch)
    check_prefix_good(x, out, ol, st, first_bad, kind, skip)
    bad = np.nonzero(st == BAD)[0]
    assert bad[0] == first_bad and (np.diff(bad) == 1).all()
    if kind == "past_in_cap":
        assert bad[-1] == n - 1
    good = np.nonzero(st == 0)[0]
    good = good[~np.isin(good, skip)]
    fl = np.concatenate([[0], np.cumsum(x.out_len)])
    assert np.array_equal(ol[good], x.want_len[good])
    assert np.array_equal(ec.gather(out, x.out_off[good], x.want_len[good]), ec.gather(x.flat, fl[good], x.want_len[good]))
    for i in skip:  # the stretched literal: the oracle's encoding of the bytes its offsets now name
        want = oracle_encode(x.blob[io[i] : io[i + 1]].tobytes())
        assert st[i] == 0 and ol[i] == len(want) <= oo[i + 1] - oo[i]
        assert out[oo[i] : oo[i] + ol[i]].tobytes() == want
    b.assert_outside_untouched(big, kind)
    codec.check()  # the failing synchronous call took the sticky flag with it
    # async: the call returns, check() reports
    codec.encode_into(b.src, dio, b.out, doo, b.ol, b.st, device=True, sync=False)
    with pytest.raises(RuntimeError, match="hpk_ctx_check"):
        codec.check()
    codec.check()
    # the same buffers with good offsets
    b.big.fill_(FILL)
    codec.encode_into(b.src, off_dev(x.in_off), b.out, off_dev(x.out_off), b.ol, b.st, device=True, sync=True)
    big, out, ol, st = b.results()
    assert not st.any() and np.array_equal(ol, x.out_len)
    assert np.array_equal(ec.gather(out, x.out_off, x.out_len), x.flat)
    b.assert_outside_untouched(big, kind + ", good offsets")


@pytest.mark.parametrize("at", ["tile_start", "mid_tile"])
def test_encode_bad_offsets_second_tile(codec, geo, at):
    """One workgroup, the bad literal in its second tile (by tile_plan): tile 0's literals are encoded and
    correct; from the bad literal on everything is HPK_BAD_OFFSETS. tile_start: the bad literal is tile 1's
    first, so all of tile 1 is void. mid_tile: tile 1's literals before it are encoded too."""
    from loona_amd import _lib

    BAD = _lib.HPK_BAD_OFFSETS
    case = ec.case("in_cut_eq-in0")
    x = ec.expected(case)
    n = len(x.in_off) - 1
    plan = tile_plan(x.in_off, x.out_off, 0, 0, geo)
    assert n <= geo.P and plan[0] == (0, HEAD, "input") and plan[1] == (HEAD, n - HEAD, "end")
    j = HEAD if at == "tile_start" else HEAD + 4
    oo = x.out_off.copy()
    assert oo[j] >= 1
    oo[j + 1] = oo[j] - 1  # literal j's region ends before it starts; the literals before j keep their offsets
    b = Buffers(x.blob, n, int(x.out_off[-1]), 0, 0)
    with pytest.raises(RuntimeError, match="hpk_encode_batch"):
        codec.encode_into(b.src, off_dev(x.in_off), b.out, off_dev(oo), b.ol, b.st, device=True, sync=True)
    big, out, ol, st = b.results()
    assert (st[:HEAD] == 0).all(), "tile 0 is void"
    check_prefix_good(x, out, ol, st, j, at)
    assert (st[j:] == BAD).all() and (ol[j:] == 0).all()
    b.assert_outside_untouched(big, at)
    assert (out[x.out_off[j] : b.total] == FILL).all()  # nothing of the void literals' regions either
    codec.check()


def test_encode_empty_batch(codec):
    """n == 0: HPK_E_OK, and nothing is touched."""
    b = Buffers(np.zeros(0, np.uint8), 0, 0, 0, 0)
    z = off_dev([0])
    for sync in (True, False):
        codec.encode_into(b.src, z, b.out, z, b.ol, b.st, device=True, sync=sync)
    codec.check()
    torch.cuda.synchronize()
    assert (b.big.cpu().numpy() == FILL).all()
    assert (b.ol.cpu().numpy() == 7).all() and (b.st.cpu().numpy() == 9).all()
