"""Placed edge cases for the small-call mode's persistent kernel (hpk_ctx_set_small_mode: hpk_persist.h, and per
literal hpk_persist_lit.h). Shared by test_persist_cases.py (CPU: every named batch holds what its name says, by the
models below) and test_gpu_persist.py (the mode against the oracle at the same regions and against the launch path,
bit for bit).

The kernel gives each literal to one lane, which takes one of four ways (dispatch()): an empty literal writes
nothing; a literal of at most slot_max bytes is staged in LDS and walked by the wave kernel's lane walk when its
region holds the decoded bound (staged_bound) or code by code with a capacity test per byte when it does not
(staged_bytes); a longer one is walked from global memory (global). A literal whose offsets are bad is not decoded
and the request goes to the launch path (bad). The staged ways store through a plan of five pieces (store_plan()):
head bytes up to the 4-aligned address, single dwords up to the 16-aligned one, 16-byte groups, trailing dwords,
tail bytes. Literal i belongs to workgroup (i // threads) mod G, thread i mod threads (owner()).

Every constant comes from hpk_test_persist_geometry, so a changed constant moves the cases. The regions here are
laid out byte-exact (loona_amd/batch.py lays them out 4-aligned, so the suite's other batches reach few of the
plan's arms); canary gaps between regions are empty literals whose regions are the gaps, the only way the ABI
has. A Batch is (blob, in_off, out_off, in_cap, out_cap, meta): int64 offsets, meta what the batch claims about
itself, for the CPU test to prove."""

import collections
import ctypes
import functools
import itertools

import numpy as np

import decode_long_cases as dc
from decode_long_cases import Stream, _seed, bound, valid, walk

Geo = collections.namedtuple("Geo", "slot_max slot_chunks out_dwords threads")
Batch = collections.namedtuple("Batch", "blob in_off out_off in_cap out_cap meta")
Expected = collections.namedtuple("Expected", "out out_len status")

SM_MAX, SM_WGS, SM_IDLE_MS = 4096, 2, 200  # test_gpu_persist.py's mode
VERDICTS = ("empty", "staged_bound", "staged_bytes", "global")
FIVE = [ord(c) for c in "012aceiost"]  # symbols with 5-bit codes
STORE_COUNTS = tuple(range(0, 21)) + tuple(range(176, 181))
IN_LENGTHS = (1, 2, 3, 4, 15, 16, 17, 97, 112, 113)
GLOBAL_LENGTHS = (114, 115, 128, 129, 2048)
FAULTS = ("p0_gt_p1", "p1_gt_in_cap", "o0_gt_o1", "o1_gt_out_cap")
IN_SLACK = 16  # bytes of a `bad` batch's input past in_off[n] (so that in_off[n - 1] > in_off[n] still lies in in_cap)


@functools.lru_cache(maxsize=None)
def geometry():
    from loona_amd import _lib

    v = [ctypes.c_uint32() for _ in range(4)]
    assert _lib.lib().hpk_test_persist_geometry(*[ctypes.byref(x) for x in v]) == _lib.HPK_E_OK
    return Geo(*[int(x.value) for x in v])


# ---- the models -------------------------------------------------------------------------------------------------

def dispatch(geo, p0, p1, o0, o1, in_mis=0, in_cap=1 << 32, out_cap=1 << 32):
    """what the kernel does with a literal (hpk_persist.h, the literal loop)"""
    if not (p0 <= p1 and p1 <= in_cap and o0 <= o1 and o1 <= out_cap):
        return "bad"
    nb, b0 = p1 - p0, p0 + in_mis
    if nb == 0:
        return "empty"
    if ((b0 + nb + 15) >> 4) - (b0 >> 4) <= geo.slot_chunks and nb <= geo.slot_max:
        return "staged_bound" if o1 - o0 >= bound(nb) else "staged_bytes"
    return "global"


def fault(p0, p1, o0, o1, in_cap, out_cap):
    """the first of the kernel's four offset tests a literal fails, or None"""
    tests = (p0 <= p1, p1 <= in_cap, o0 <= o1, o1 <= out_cap)
    return None if all(tests) else FAULTS[tests.index(False)]


Plan = collections.namedtuple("Plan", "head lead groups trail tail")


def store_plan(ob, cnt):
    """the pieces persist_literal_lds stores cnt bytes at ob with: head bytes, leading dwords, 16-byte groups,
    trailing dwords, tail bytes"""
    e = ob + cnt
    h = min((ob + 3) & ~3, e)
    t = max(e & ~3, h)
    h16 = min((h + 15) & ~15, t)
    t16 = max(t & ~15, h16)
    return Plan(h - ob, (h16 - h) // 4, (t16 - h16) // 16, (t - t16) // 4, e - t)


def owner(geo, i, G):
    """(workgroup, thread, round) of literal i: i = wg * threads + tid, += G * threads"""
    return (i // geo.threads) % G, i % geo.threads, i // (G * geo.threads)


def verdicts(geo, b, in_mis=0):
    io, oo = b.in_off, b.out_off
    return [dispatch(geo, int(io[i]), int(io[i + 1]), int(oo[i]), int(oo[i + 1]), in_mis, b.in_cap, b.out_cap)
            for i in range(len(io) - 1)]


# ---- the builder ------------------------------------------------------------------------------------------------

class Builder:
    """literals and regions laid end to end; gap(k): an empty literal whose region is k canary bytes"""

    def __init__(self, rng):
        self.rng, self.lits, self.caps, self.ip, self.op = rng, [], [], 0, 0

    def add(self, lit, cap=None):
        self.lits.append(bytes(lit))
        self.caps.append(bound(len(lit)) if cap is None else int(cap))
        assert self.caps[-1] >= 0
        self.ip += len(lit)
        self.op += self.caps[-1]
        return len(self.lits) - 1

    def gap(self, k):
        return self.add(b"", k)

    def out_to(self, res, mod=16, least=1):
        """a canary gap of at least `least` bytes up to the next output address that is res mod `mod`"""
        k = (res - self.op) % mod
        while k < least:
            k += mod
        self.gap(k)

    def in_to(self, res):
        """a short valid literal up to the next input address that is res mod 16"""
        p = (res - self.ip) % 16
        if p:
            self.add(valid(p, self.rng))

    def batch(self, meta, in_slack=0):
        lens = np.fromiter((len(x) for x in self.lits), np.int64, len(self.lits))
        io = np.zeros(len(lens) + 1, np.int64)
        np.cumsum(lens, out=io[1:])
        oo = np.zeros(len(lens) + 1, np.int64)
        np.cumsum(np.asarray(self.caps, np.int64), out=oo[1:])
        blob = np.frombuffer(b"".join(self.lits) + b"\xff" * in_slack, np.uint8).copy()
        return Batch(blob, io, oo, int(blob.size), int(oo[-1]), meta)


def five(count, rng):
    """a literal of `count` 5-bit codes and ones to the byte's end; count 0: one byte of ones (no symbol, status 1)"""
    if count == 0:
        return b"\xff"
    s = Stream(rng)
    for j in rng.integers(0, len(FIVE), count):
        s.sym(FIVE[int(j)])
    return s.raw("1" * (-s.n % 8)).bytes()


def text_eos(m, nbytes, rng):
    """m text symbols, EOS, random bytes up to nbytes: status 3 after m bytes"""
    s = Stream(rng)
    for _ in range(m):
        s.sym(s.pick(int(rng.integers(5, 9))))
    return s.eos().random_to(nbytes).bytes()


def text_cut(nbytes, rng):
    """text, then the first 13 bits of a 30-bit code: status 1 (more than 7 bits left over)"""
    s = Stream(rng)
    return s.fill_to(8 * nbytes - 13).raw("1" * 13).bytes()


def text_bad_pad(nbytes, rng):
    """text, then four bits with a zero that hold no code: status 2"""
    s = Stream(rng)
    return s.fill_to(8 * nbytes - 4).raw("1101").bytes()


def text_pad8(nbytes, rng):
    """text ending on a byte boundary, then a byte of ones: status 1"""
    s = Stream(rng)
    return s.fill_to(8 * nbytes - 8).raw("1" * 8).bytes()


ERROR_MIX = (("eos", 3, lambda nb, rng: text_eos(max(0, nb // 3 - 2), nb, rng)), ("cut", 1, text_cut),
             ("bad_pad", 2, text_bad_pad), ("pad8", 1, text_pad8))


def store_plan_batch(geo):
    rng = _seed("persist-store-plan")
    b, rows = Builder(rng), []
    for res in range(16):
        for count in STORE_COUNTS:
            b.out_to(res)
            rows.append((b.add(five(count, rng)), res, count))
    return b.batch({"rows": rows})


def in_place_batch(geo):
    rng = _seed("persist-in-place")
    b, rows = Builder(rng), []
    for res in range(16):
        for nb in IN_LENGTHS:
            b.in_to(res)
            b.out_to(int(rng.integers(0, 16)))
            rows.append((b.add(valid(nb, rng)), res, nb))
    return b.batch({"rows": rows})


def _short_caps(count, bnd):
    caps = {"zero": 0, "minus1": count - 1, "count": count, "between": (count + bnd) // 2, "bound_minus1": bnd - 1}
    assert 0 < count - 1 and count < caps["between"] < bnd - 1, (count, bnd)  # (every capacity exists and is its own)
    return caps


def short_regions_batch(geo):
    """rows of (index, decoded count, capacity, the literal's own status, the status expected at that capacity)"""
    rng = _seed("persist-short-regions")
    b, rows = Builder(rng), []
    lits = [(valid(nb, rng), 0) for nb in (12, 40, geo.slot_max)]
    lits += [(make(nb, rng), st) for nb in (24, geo.slot_max) for _, st, make in ERROR_MIX]
    for lit, st in lits:
        w = walk(lit)
        assert w.status == st
        for which, cap in _short_caps(len(w.syms), bound(len(lit))).items():
            b.out_to(int(rng.integers(0, 16)))
            # the overflow wins while more symbols come than the region holds; at the count the literal's status
            rows.append((b.add(lit, cap), len(w.syms), cap, st, 4 if cap < len(w.syms) else st, which))
    return b.batch({"rows": rows})


GLOBAL_CAPS = ("bound", "count", "minus1", "minus2", "zero")


def global_batch(geo):
    rng = _seed("persist-global")
    b, rows = Builder(rng), []
    k = 0
    for nb in GLOBAL_LENGTHS:
        assert nb > geo.slot_max
        for res in range(8):
            for which in GLOBAL_CAPS:
                kind = k % 5
                lit, st = (valid(nb, rng), 0) if kind else (text_eos(nb // 2, nb, rng), 3)
                count = len(walk(lit).syms)
                assert count >= 2
                cap = {"bound": bound(nb), "count": count, "minus1": count - 1, "minus2": count - 2, "zero": 0}[which]
                b.in_to((3 * k) % 16)
                b.out_to(res, 8)
                rows.append((b.add(lit, cap), nb, res, which, count, 4 if cap < count else st))
                k += 1
    return b.batch({"rows": rows})


def _of_verdict(geo, v, k, rng):
    """(literal, capacity) that the kernel treats as verdict v, the k-th of its kind: the staged ones rotate through
    valid text and the error mix"""
    if v == "empty":
        return b"", k % 4
    if v == "global":
        nb = geo.slot_max + 1 + k % 27
        return (valid(nb, rng) if k % 3 else text_cut(nb, rng)), bound(nb)
    nb = 9 + (7 * k) % 52
    kind = k % (len(ERROR_MIX) + 2)
    lit = valid(nb, rng) if kind == 0 else rng.integers(0, 256, nb, dtype=np.uint8).tobytes() if kind == 1 else \
        ERROR_MIX[kind - 2][2](nb, rng)
    if v == "staged_bound":
        return lit, bound(nb)
    return lit, min(bound(nb) - 1, max(0, len(walk(lit).syms) - (k // 6) % 2))  # below the bound: the count, or one less


def mixed_wave_batch(geo):
    """512 literals: in every wave the four verdicts in an order in which each follows each (itself included)"""
    rng = _seed("persist-mixed-wave")
    # a cycle through every ordered pair of verdicts (an Euler circuit of the complete digraph with loops): 16 steps
    cyc = [0, 0, 1, 0, 2, 0, 3, 1, 1, 2, 1, 3, 2, 2, 3, 3]
    assert {(cyc[i], cyc[(i + 1) % 16]) for i in range(16)} == set(itertools.product(range(4), repeat=2))
    b, seen = Builder(rng), collections.Counter()
    for i in range(2 * geo.threads):
        v = VERDICTS[cyc[(i + i // 64) % 16]]  # (each wave starts one step further into the cycle)
        lit, cap = _of_verdict(geo, v, seen[v], rng)
        seen[v] += 1
        b.add(lit, cap)
    return b.batch({"cycle": cyc})


@functools.lru_cache(maxsize=1)
def _count_pool():
    rng = _seed("persist-counts")
    return [valid(int(rng.integers(1, 31)), rng) for _ in range(61)] + [text_cut(9, rng), text_eos(2, 12, rng), b""]


def counts_batch(n):
    """n literals from a small pool of short ones (three with errors, one empty), byte-exact regions"""
    pool = _count_pool()
    b = Builder(None)
    for i in range(n):
        b.add(pool[(i * 7 + i // 64) % len(pool)])
    return b.batch({"n": n})


def count_list(geo, G, sm_max):
    t = geo.threads
    return sorted({1, 63, 64, 65, t - 1, t, t + 1, G * t - 1, G * t, G * t + 1, sm_max})


def bad_batch(geo, which, where, G=SM_WGS):
    """600 short literals, literal `where` (first / last / wg1: one that workgroup 1 takes) with the offset fault
    `which`; the input has IN_SLACK bytes past in_off[n]"""
    n = 600
    base = counts_batch(n)
    i = {"first": 0, "last": n - 1, "wg1": geo.threads + 5}[where]
    io, oo = base.in_off.copy(), base.out_off.copy()
    in_cap, out_cap = int(io[-1]) + IN_SLACK, int(oo[-1])
    if which == "p0_gt_p1":
        io[i] = io[i + 1] + 1
    elif which == "p1_gt_in_cap":
        io[i + 1] = in_cap + 1
    elif which == "o0_gt_o1":
        oo[i] = oo[i + 1] + 1
    else:
        assert which == "o1_gt_out_cap"
        oo[i + 1] = out_cap + 1
    blob = np.concatenate([base.blob, np.full(IN_SLACK, 0xFF, np.uint8)])
    return Batch(blob, io, oo, in_cap, out_cap, {"literal": i, "fault": which, "G": G})


def _table(geo):
    t = {"store_plan": lambda: store_plan_batch(geo), "in_place": lambda: in_place_batch(geo),
         "short_regions": lambda: short_regions_batch(geo), "global": lambda: global_batch(geo),
         "mixed_wave": lambda: mixed_wave_batch(geo)}
    for n in count_list(geo, SM_WGS, SM_MAX):
        t[f"counts-{n}"] = lambda n=n: counts_batch(n)
    t["over_max"] = lambda: counts_batch(SM_MAX + 1)
    for which in FAULTS:
        for where in ("first", "last", "wg1"):
            t[f"bad-{which}-{where}"] = lambda a=which, b=where: bad_batch(geo, a, b)
    return t


GOOD_NAMES = ("store_plan", "in_place", "short_regions", "global", "mixed_wave")
BAD_NAMES = tuple(f"bad-{w}-{p}" for w in FAULTS for p in ("first", "last", "wg1"))


def names():
    return tuple(_table(geometry()))


@functools.lru_cache(maxsize=None)
def batch(name):
    """the named batch (kept: shared between tests and never modified)"""
    return _table(geometry())[name]()


def oracle_regions(b):
    """the oracle on a batch with the caller's regions: (out_cap bytes prefilled with 0xAB, out_len, status)"""
    from hpk_util import oracle

    n = len(b.in_off) - 1
    io = np.ascontiguousarray(b.in_off, np.uint32)
    oo = np.ascontiguousarray(b.out_off, np.uint32)
    out = np.full(max(b.out_cap, 1), 0xAB, np.uint8)
    ol = np.zeros(max(n, 1), np.uint32)
    st = np.zeros(max(n, 1), np.uint8)
    src = b.blob if b.blob.size else np.zeros(1, np.uint8)
    oracle().oracle_decode_batch(src.ctypes.data, io.ctypes.data, n, out.ctypes.data, oo.ctypes.data, ol.ctypes.data,
                                 st.ctypes.data, 8)
    return Expected(out[: b.out_cap], ol[:n].astype(np.int64), st[:n])


@functools.lru_cache(maxsize=None)
def expected_of(name):
    return oracle_regions(batch(name))


def valid_bytes(out, out_off, out_len):
    """every literal's first out_len bytes end to end"""
    return dc.gather(out, out_off, out_len)
