"""Placed edge cases for the two decode phases behind the fills: the long-literal phase (hpk_long.h, one lane per
literal of >= 64 encoded bytes through an LDS ring) and the huge-literal phase (hpk_huge.h / hpk_huge_piece.h, a
literal of >= 8 KiB walked speculatively in pieces by a whole workgroup, with fix rounds). Shared by
test_decode_long_cases.py (CPU: every case reaches the edge it is named for, and the huge phase's replay in
tests/emu/emu.cpp decodes it as the oracle does under the 12-bit and the 13-bit table) and
test_gpu_decode_long.py (both kernels, every output form, against the oracle bit for bit).

The cases are built from tests/golden/huffman_table.json with a bit-level builder (Stream: a chosen code at a
chosen bit position, codes of chosen lengths up to it, an ending as asked) and placed against the kernels' own
constants (hpk_test_decode_geometry). huge_geometry() restates hpk_huge_piece.h's piece geometry, blocks() and
wg_range() the launch's workgroup count and a workgroup's literal range (hpk_decode.hip, hpk_wave.h), walk() is
a plain RFC 7541 decoder that also gives every code's bit position: the tests use it, not the replay, to prove
where a case's code starts.

A case is Case(lits, caps, meta): the batch's literals, each literal's output capacity (None: its decoded
bound, regions back to back), and what the case claims about itself. Sizes: 8,192 B is the smallest huge literal
(P = 128 pieces of PB = 64 bytes), 65,536 B the smallest that uses all 1024 lanes. The lead OV switches from 256
to 512 bits where PB reaches 512, which by huge_geometry is between 523,264 B (PB 511) and 523,265 B; the two
`ov-` cases are 523,264 B and 524,288 B.

Two families are narrower than their names:
  * long-short-output: a literal of >= 64 bytes that decodes m symbols and then meets a cut long code exists
    for m = 17 only (seventeen 30-bit codes are 510 bits); m = 0, 1, 15, 16 end in EOS alone;
  * long-claims: a workgroup's range never holds more than 64 literals unless the grid is capped by the device's
    CUs (hpk_decode.hip: ceil(n / 64) workgroups at least), so the counts above 64 are per range of a batch of
    count x CUs literals, which the cap splits into CUs ranges of `count` each."""

import collections
import ctypes
import functools
import struct

import numpy as np

from hpk_util import load

TABLE = [(int(c), int(l)) for c, l in load("huffman_table.json")["table"]]  # [code, bits] per symbol, EOS last
EOS = 256
BITS = [format(c, "0%db" % l) for c, l in TABLE]
LEN = [l for _, l in TABLE]
BY_LEN = {}
for _s in range(256):
    BY_LEN.setdefault(LEN[_s], []).append(_s)
DEC = {}
for _s in range(257):
    DEC.setdefault(LEN[_s], {})[BITS[_s]] = _s
LENS = sorted(DEC)
CUS_MAX = 256  # the CUs of one device, for the plan test (the GPU test passes the device's own count)

Case = collections.namedtuple("Case", "lits caps meta")
Geo = collections.namedtuple("Geo", "block huge_min huge_max piece_min long_min long_big ring chunks steps claim "
                                    "waves obuf table")


@functools.lru_cache(maxsize=None)
def geometry(kind="wave"):
    from loona_amd import _lib

    v = (ctypes.c_uint32 * 13)()
    assert _lib.lib().hpk_test_decode_geometry({"fill": 1, "wave": 2}[kind], v) == _lib.HPK_E_OK
    return Geo(*[int(x) for x in v])


def huge_geometry(nbytes, lanes, piece_min):
    """(P, PB, OV) of hpk_huge_piece.h: P pieces of PB bytes (the last one shorter, never empty), OV bits of lead"""
    P = min(lanes, (nbytes + piece_min - 1) // piece_min)
    PB = (nbytes + P - 1) // P
    P = (nbytes + PB - 1) // PB
    return P, PB, 512 if PB >= 512 else 256


def blocks(n, in_cap, cus):
    """the workgroups of a decode launch (hpk_decode.hip, decode_blocks)"""
    return max(1, min(max((n + 63) // 64, (in_cap + 32767) // 32768), n, cus))


def wg_range(n, g, w):
    """workgroup w of g: its literals [BA, BB)"""
    return n * w // g, n * (w + 1) // g


def bound(nbytes):
    return 8 * int(nbytes) // 5


Walk = collections.namedtuple("Walk", "starts syms status end")


def walk(lit):
    """RFC 7541 5.2 decode of one literal, code by code (huffman.rs:95-161): the bit position and the symbol of
    every code decoded, the status (0 ok, 1 more than 7 bits left over, 2 left-over bits not all ones, 3 EOS
    decoded) and the bit position where the walk stopped."""
    s = bin(int.from_bytes(b"\x01" + bytes(lit), "big"))[3:]
    n, p, starts, syms = len(s), 0, [], []
    while True:
        sym = None
        for l in LENS:
            if p + l > n:
                break
            sym = DEC[l].get(s[p : p + l])
            if sym is not None:
                break
        if sym is None:
            break
        if sym == EOS:
            return Walk(starts, syms, 3, p)
        starts.append(p)
        syms.append(sym)
        p += l
    return Walk(starts, syms, 1 if n - p > 7 else 2 if "0" in s[p:] else 0, p)


def _feasible(n):
    return n == 0 or 5 <= n <= 8 or n >= 10


@functools.lru_cache(maxsize=None)
def _split(need):
    """code lengths of 5 to 8 bits that sum to `need`"""
    assert _feasible(need), need
    if need == 0:
        return ()
    if need <= 8:
        return (need,)
    for l in (6, 7, 5, 8):
        if _feasible(need - l):
            return (l,) + _split(need - l)
    raise AssertionError(need)


class Stream:
    """A literal under construction, bit by bit. n: its bits so far; count: the symbols a decoder gets from them."""

    def __init__(self, rng):
        self.parts, self.n, self.count, self.rng, self._draws = [], 0, 0, rng, []

    def sym(self, s):
        self.parts.append(BITS[s])
        self.n += LEN[s]
        self.count += 1
        return self

    def syms(self, it):
        for s in it:
            self.sym(s)
        return self

    def eos(self):
        self.parts.append(BITS[EOS])
        self.n += 30
        return self

    def raw(self, bits):
        self.parts.append(bits)
        self.n += len(bits)
        return self

    def pick(self, l):
        """a symbol whose code has l bits (random numbers drawn 512 at a time: a draw per symbol is slow)"""
        if not self._draws:
            self._draws = self.rng.integers(0, 1 << 30, 512).tolist()
        syms = BY_LEN[l]
        return syms[self._draws.pop() % len(syms)]

    def fill_to(self, pos, lens=(5, 6, 7, 8)):
        """codes of the given lengths in turn up to bit `pos` exactly (the last few of 5 to 8 bits, as the sum needs)"""
        assert _feasible(pos - self.n), (pos, self.n)
        i = 0
        while pos - self.n >= lens[i % len(lens)] + 40:
            self.sym(self.pick(lens[i % len(lens)]))
            i += 1
        for l in _split(pos - self.n):
            self.sym(self.pick(l))
        return self

    def cycle_to(self, pos, cyc):
        """the symbols of `cyc` in turn while the next one ends at or before bit `pos`"""
        i = 0
        while self.n + LEN[cyc[i % len(cyc)]] <= pos:
            self.sym(cyc[i % len(cyc)])
            i += 1
        return self

    def finish(self, nbytes, lens=(5, 6, 7, 8)):
        """a valid end at nbytes: codes up to 0..7 bits before it, then ones"""
        tot = 8 * nbytes
        if tot - self.n > 7 or tot - self.n < 0:
            pads = [p for p in range(8) if tot - p >= self.n and _feasible(tot - p - self.n)]
            assert pads, (nbytes, self.n)
            self.fill_to(tot - pads[int(self.rng.integers(0, len(pads)))], lens)
        return self.raw("1" * (tot - self.n))

    def random_to(self, nbytes):
        """ones to the next byte boundary, then random bytes up to nbytes"""
        self.raw("1" * (-self.n % 8))
        k = nbytes - self.n // 8
        assert k >= 0
        return self.raw("".join(format(int(b), "08b") for b in self.rng.integers(0, 256, k)))

    def bytes(self):
        s = "".join(self.parts)
        assert len(s) % 8 == 0 and len(s) == self.n
        return int(s, 2).to_bytes(len(s) // 8, "big") if s else b""


def _seed(name):
    """a seed from a case's name that does not depend on the interpreter's string hashing"""
    return np.random.default_rng(list(name.encode()))


def valid(nbytes, rng, lens=(5, 6, 7, 8)):
    return Stream(rng).finish(nbytes, lens).bytes()


def one_byte(rng):
    return valid(1, rng)


# ---- the huge phase ---------------------------------------------------------------------------------

# Streams that a walk which starts off a code boundary does not find its way back into: (symbols in front, the
# cycle repeated). Measured with the replay (tests/emu/emu.cpp), 128 pieces: 127 fix rounds each, but
#   * an 8-bit code repeated from bit 0 needs none: the pieces and their leads start on byte boundaries, which
#     are its code boundaries; behind one 5-bit code 'X' and 'Z' need 127, '&', '*', ',' and ';' still none
#     (their streams pull every walk back in);
#   * byte 10 with '0' (28 ones and 7 zeros) pulls every walk back in within the lead: 0 rounds whatever stands
#     in front. It stays among the noresync cases as a stream of long codes that does resynchronise
#     (RESYNCS); byte 22 with '0' (29 ones and 6 zeros) is the cycle of that kind that does not.
NORESYNC = {
    "len5": ((), (ord("0"),)),
    "len6": ((), (ord("A"),)),
    "len7": ((), (ord("x"),)),
    "len8": ((ord("0"),), (ord("X"),)),
    "len30": ((), (10,)),
    "cyc01": ((), (ord("0"), ord("1"))),
    "cyc10_0": ((), (10, ord("0"))),
    "cyc22_0": ((), (22, ord("0"))),
}
RESYNCS = ("cyc10_0",)
# the foreign symbol in the middle: its length is no multiple of the cycle's, and walks do not merge on it
NORESYNC_FOREIGN = {"len5": ord(" "), "len6": ord("1"), "len7": ord("0"), "len8": ord("0"), "len30": ord("0"),
                    "cyc01": ord(" "), "cyc10_0": ord(" "), "cyc22_0": ord(" ")}
NORESYNC_ENDINGS = ("clean", "foreign", "eos")
# Cycles of long codes in whose stream a walk from a wrong bit meets 30 ones (EOS) inside a piece's lead, so that
# pass 1 leaves the piece without a start: found by a search over cycles of up to three codes of 20 to 30 bits
# with the replay (the streams' own walk never meets EOS). The first has such pieces here and there, the second
# runs of them.
NONE_CHAIN = {"none-chain-1": ((13, 196), ()), "none-chain-2": ((249, 172), ())}


def sizes(geo):
    """(the smallest huge literal, the smallest that uses every lane)"""
    return geo.huge_min, geo.block * geo.piece_min


def noresync(geo, stream, size, ending):
    lead, cyc = NORESYNC[stream]
    s = Stream(_seed("noresync")).syms(lead)
    tot = 8 * size
    if ending == "foreign":
        s.cycle_to(tot // 2, cyc).sym(NORESYNC_FOREIGN[stream])
    elif ending == "eos":
        s.cycle_to(3 * tot // 4, cyc).eos()
    s.cycle_to(tot, cyc)
    while tot - s.n > 7:
        s.sym(ord("0"))
    lit = s.raw("1" * (tot - s.n)).bytes()
    P, PB, _ = huge_geometry(size, geo.block, geo.piece_min)
    return Case([lit], None, {"P": P, "status": 3 if ending == "eos" else 0})


def none_chain(geo, name):
    cyc, lead = NONE_CHAIN[name]
    s = Stream(_seed(name)).syms(lead).cycle_to(8 * geo.huge_min - 40, cyc)
    return Case([s.finish(geo.huge_min).bytes()], None, {"status": 0})


def _nx(geo):
    """the bit where piece 2 of the smallest huge literal starts"""
    _, PB, _ = huge_geometry(geo.huge_min, geo.block, geo.piece_min)
    return 2 * PB * 8


def straddle(geo, bits, d):
    """a code of `bits` bits that starts d bits before the boundary between pieces 1 and 2"""
    name = f"straddle{bits}-d{d}"
    s = Stream(_seed(name))
    s.fill_to(_nx(geo) - d).sym(s.pick(bits))
    return Case([s.finish(geo.huge_min).bytes()], None, {"bit": _nx(geo) - d, "len": bits, "status": 0})


def pair_on_boundary(geo, l0, l1, rel):
    """behind a 13-bit code (so a table lookup starts there), a code of l0 bits and one of l1 bits: one table
    entry holds both; the second starts `rel` bits from the boundary between pieces 1 and 2"""
    s = Stream(_seed(f"pair{l0}{l1}{rel}"))
    at = _nx(geo) + rel
    s.fill_to(at - l0 - 13).sym(s.pick(13)).sym(s.pick(l0)).sym(s.pick(l1))
    return Case([s.finish(geo.huge_min).bytes()], None, {"bit": at, "len": l1, "first_len": l0, "status": 0})


def eos_at(geo, where):
    s = Stream(_seed(f"eos-at-{where}"))
    P, PB, _ = huge_geometry(geo.huge_min, geo.block, geo.piece_min)
    at = (P - 1) * PB * 8 + 100 if where == "last" else _nx(geo) + where
    s.fill_to(at).eos()
    return Case([s.random_to(geo.huge_min).bytes()], None, {"bit": at, "status": 3})


def last_piece_size(geo, last):
    """the smallest literal of more than 130 pieces whose last piece has `last` bytes (8,321 B for 1)"""
    for nb in range(geo.huge_min + 2 * geo.piece_min, geo.huge_min + 4096):
        P, PB, _ = huge_geometry(nb, geo.block, geo.piece_min)
        if nb - (P - 1) * PB == last:
            return nb
    raise AssertionError(last)


def last_piece(geo, last, ending):
    nb = last_piece_size(geo, last)
    P, PB, _ = huge_geometry(nb, geo.block, geo.piece_min)
    st, tot = (P - 1) * PB * 8, 8 * nb
    s = Stream(_seed(f"last-piece-{last}-{ending}"))
    if ending == "valid":
        s.finish(nb)
        status = 0
    elif ending == "ones8":
        s.fill_to(tot - 8).raw("1" * 8)
        status = 1
    elif ending == "zero":
        s.fill_to(tot - 4).raw("1101")
        status = 2
    else:  # a 30-bit code from 25 bits before the last piece to 5 bits into it, then ones: nothing starts in the piece
        assert ending == "padonly"
        s.fill_to(st - 25).sym(s.pick(30)).raw("1" * (tot - st - 5))
        status = 0 if tot - st - 5 <= 7 else 3
    return Case([s.bytes()], None, {"bytes": nb, "last": last, "status": status, "c0": ending == "padonly"})


def terminal_early(geo):
    s = Stream(_seed("terminal-early"))
    _, PB, _ = huge_geometry(geo.huge_min, geo.block, geo.piece_min)
    at = PB * 8 + 88  # inside piece 1
    s.fill_to(at).eos()
    return Case([s.random_to(geo.huge_min).bytes()], None, {"bit": at, "status": 3})


def ov_case(geo, pb):
    """text with a code of 19 to 30 bits every few dozen symbols (walks find their way back slowly), P = the
    block's lanes, PB = pb"""
    nb = geo.block * pb
    s = Stream(_seed(f"ov{pb}"))
    lens = (5, 6, 7, 6, 5, 8, 6, 7, 5, 6, 28, 6, 5, 7, 6, 5, 6, 30, 7, 6, 5, 19, 6, 7)
    return Case([s.finish(nb, lens).bytes()], None, {"bytes": nb, "pb": pb, "status": 0})


def one_range(huge_lits, rng, cus=CUS_MAX):
    """the huge literals as the whole of workgroup 0's range: one-byte literals behind them bring the batch to
    len(huge_lits) x (its workgroups)"""
    h = len(huge_lits)
    tot = sum(len(x) for x in huge_lits)
    for g in range(1, cus + 1):
        n = h * g
        if blocks(n, tot + n - h, cus) == g:
            return list(huge_lits) + [one_byte(rng) for _ in range(n - h)]
    raise AssertionError("no batch puts these literals into one range")


def share(geo, kind):
    rng = _seed(f"share-{kind}")
    small, full = sizes(geo)
    per = geo.block // huge_geometry(small, geo.block, geo.piece_min)[0]  # literals of the smallest size per round
    if kind == "exact":
        nbs = [small] * per
    elif kind == "plus1":
        nbs = [small] * (per + 1)
    elif kind == "full_then_small":
        nbs = [full, small]
    else:
        assert kind == "list_plus1"
        nbs = [small] * (geo.huge_max + 1)
    lits = one_range([valid(nb, rng) for nb in nbs], rng)
    return Case(lits, None, {"huge": len(nbs), "P": [huge_geometry(nb, geo.block, geo.piece_min)[0] for nb in nbs]})


CAPACITIES = ("bound", "exact", "minus1", "7")


def capacity(geo, nbytes, which):
    """a valid text literal of nbytes between two short ones, its region the decoded bound, the decoded size,
    one byte less, or 7 bytes"""
    rng = _seed(f"capacity-{nbytes}")
    s = Stream(rng).finish(nbytes)
    lit, dec = s.bytes(), s.count
    cap = {"bound": bound(nbytes), "exact": dec, "minus1": dec - 1, "7": 7}[which]
    lits = [valid(9, rng), lit, valid(11, rng)]
    return Case(lits, [bound(9), cap, bound(11)], {"decoded": dec, "cap": cap, "bytes": nbytes})


# ---- the long phase ------------------------------------------------------------------------------------

SWEEP_STREAMS = ("five", "thirty", "text", "alternate")


def long_stream(kind, nbytes, rng):
    """(literal, decoded size): a valid literal of exactly nbytes of 5-bit codes only (it fills its decoded bound),
    of 30-bit codes (and the few 5-bit ones the end needs), of text, or of 5- and 30-bit codes in turn"""
    s = Stream(rng)
    tot = 8 * nbytes
    if kind == "five":
        while s.n + 5 <= tot:
            s.sym(s.pick(5))
    elif kind == "text":
        s.finish(nbytes)
    else:
        i = 0
        while True:
            l = 30 if kind == "thirty" or i % 2 else 5
            if s.n + l > tot:
                break
            s.sym(s.pick(l))
            i += 1
        while tot - s.n > 7:
            s.sym(s.pick(5))
    return s.raw("1" * (tot - s.n)).bytes(), s.count


def _align_in(lits, off, want, rng):
    """a short valid literal in front, so that the next literal starts at `want` mod 16; the new offset"""
    p = (want - off) % 16
    if p:
        lits.append(valid(p, rng))
    return off + p


def long_sweep(geo):
    """every encoded length long_min .. 208 x every in_off mod 16 x four streams, exact-bound regions back to back"""
    rng = _seed("long-sweep")
    lits, rows, off = [], [], 0
    for nb in range(geo.long_min, 209):
        for al in range(16):
            for kind in SWEEP_STREAMS:
                off = _align_in(lits, off, al, rng)
                lit, dec = long_stream(kind, nb, rng)
                rows.append((len(lits), nb, al, dec))
                lits.append(lit)
                off += nb
    return Case(lits, None, {"rows": rows})


def ring_lengths(geo):
    per = 16 * geo.chunks  # bytes per refill
    out = []
    for k in range(2, 13):
        out += [per * k - 1, per * k, per * k + 1]
    return out + [4 * geo.ring - 1, 4 * geo.ring, 4 * geo.ring + 1, geo.huge_min - 1]


def long_ring(geo):
    rng = _seed("long-ring")
    lits, rows = [], []
    for nb in ring_lengths(geo):
        for kind in ("thirty", "five"):
            lit, dec = long_stream(kind, nb, rng)
            rows.append((len(lits), nb, None, dec))
            lits.append(lit)
    return Case(lits, None, {"rows": rows})


SHORT_OUTPUTS = ((0, "eos"), (1, "eos"), (15, "eos"), (16, "eos"), (17, "eos"), (17, "cut"))


def long_short_output(geo):
    """literals of >= long_min bytes that decode m bytes: m text symbols and EOS, random bytes behind; or seventeen
    30-bit codes and ten bits of an eighteenth. Each at every out_off mod 16 (one-byte literals, bound 1, in front)."""
    rng = _seed("long-short-output")
    lits, rows, oo = [], [], 0
    for m, how in SHORT_OUTPUTS:
        for al in range(16):
            while oo % 16 != al:
                lits.append(one_byte(rng))
                oo += 1
            s = Stream(rng)
            if how == "eos":
                for _ in range(m):
                    s.sym(s.pick(int(rng.integers(5, 9))))
                nb = geo.long_min + int(rng.integers(0, 40))
                lit = s.eos().random_to(nb).bytes()
            else:
                for _ in range(m):
                    s.sym(s.pick(30))
                lit = s.raw("1" * 10).bytes()
                assert len(lit) >= geo.long_min
            rows.append((len(lits), m, al, 3 if how == "eos" else 1))
            lits.append(lit)
            oo += bound(len(lit))
    return Case(lits, None, {"rows": rows})


BAD_PADS = {1: "0", 2: "10", 3: "110", 4: "1101", 5: "11110", 6: "111110", 7: "1111101"}
TAIL_BYTES = 97


def long_tail(geo):
    """a text body, then every ending within the last 35 bits: rows of (index, what, status)"""
    rng = _seed("long-tail")
    tot = 8 * TAIL_BYTES
    lits, rows = [], []

    def add(what, status, tail_bits, tail):
        s = Stream(rng).fill_to(tot - tail_bits)
        tail(s)
        assert s.n == tot
        rows.append((len(lits), what, status))
        lits.append(s.bytes())

    for p in range(8):
        add(f"pad{p}", 0, p, lambda s, p=p: s.raw("1" * p))
    for p, bits in BAD_PADS.items():
        add(f"zero-in-pad{p}", 2, p, lambda s, bits=bits: s.raw(bits))
    for r in range(8, 30):  # the first r bits of a 30-bit code
        add(f"cut{r}", 1, r, lambda s, r=r: s.raw("1" * r))
    for l in [x for x in LENS if x >= 13]:
        add(f"code{l}-ends", 0, l, lambda s, l=l: s.sym(s.pick(l)))
    add("eos-ends", 3, 30, lambda s: s.eos())
    return Case(lits, None, {"rows": rows})


CLAIM_COUNTS = (63, 64, 65, 128, 129, 511, 512, 513, 1025)


@functools.lru_cache(maxsize=1)
def _claim_pool(long_min, long_big):
    rng = _seed("claim-pool")
    small = [valid(int(rng.integers(long_min, 161)), rng) for _ in range(96)]
    big = [valid(int(rng.integers(long_big, long_big + 200)), rng) for _ in range(8)]
    short = [valid(int(rng.integers(long_min - 8, long_min)), rng) for _ in range(64)]
    return small, big, short


def long_claims(geo, count, sprinkled, cus=CUS_MAX):
    """`count` long literals in a workgroup's range, a few of them of >= long_big bytes; sprinkled: each behind two
    literals just below long_min (more short bytes than long ones in the range's first 2,048 literals, so the
    range is not listed whole). One workgroup for the counts up to 64. Else the grid is capped by the CUs and the
    batch has `cus` ranges of equally many literals: the first, the middle and the last range are such ranges,
    the others hold one-byte literals (the batch stays small)."""
    small, big, short = _claim_pool(geo.long_min, geo.long_big)
    rng = _seed(f"long-claims-{count}-{sprinkled}")
    one_wg = (3 * count if sprinkled else count) <= 64
    pool = small + big + short + [bytes([8 * i + 7]) for i in range(10)]  # (a 5-bit code and three ones)
    tiny0 = len(small) + len(big) + len(short)
    nbig = 4 if count >= 256 else 1 if sprinkled else 2  # (few: the batch's bytes stay small)
    # (sprinkled: long literals of at most 100 bytes, so that two short ones in front outweigh each)
    few = np.array([i for i, x in enumerate(small) if not sprinkled or len(x) <= 100])
    ranges = 1 if one_wg else cus
    ids = []
    for w in range(ranges):
        if w not in (0, ranges // 2, ranges - 1):
            ids.append(tiny0 + rng.integers(0, 10, 3 * count if sprinkled else count))
            continue
        lo = few[rng.integers(0, len(few), count)]
        lo[rng.choice(count, nbig, replace=False)] = len(small) + rng.integers(0, len(big), nbig)
        if sprinkled:
            r = np.empty(3 * count, np.int64)
            r[0::3] = len(small) + len(big) + rng.integers(0, len(short), count)
            r[1::3] = len(small) + len(big) + rng.integers(0, len(short), count)
            r[2::3] = lo
            lo = r
        ids.append(lo)
    lits = [pool[i] for i in np.concatenate(ids)]
    return Case(lits, None, {"count": count, "one_wg": one_wg, "cus": cus})


# ---- independence from neighbouring bytes -----------------------------------------------------------------------

def neighbour(geo, which, mod):
    """[a literal in front, the literal under test], the batch ending at in_cap with in_cap mod 16 == mod. The
    test varies the front literal's last byte and the bytes behind in_cap; the second literal must not change.
    which: long / huge, ending valid or in a cut 30-bit code"""
    rng = _seed(f"neighbour-{which}-{mod}")
    kind, end = which.split("_")
    nb = 200 if kind == "long" else geo.huge_min
    s = Stream(rng)
    if end == "valid":
        s.finish(nb)
    else:
        s.fill_to(8 * nb - 13).raw("1" * 13)
    lit = s.bytes()
    front = valid((mod - nb) % 16 + 16, rng)
    assert (len(front) + nb) % 16 == mod
    return Case([front, lit], None, {"status": 0 if end == "valid" else 1})


NEIGHBOURS = ("long_valid", "long_cut", "huge_valid", "huge_cut")


# ---- the cases by name -------------------------------------------------------------------------------------------

def _case_table(geo, cus):
    t = {}
    small, full = (8192, 65536) if geo is None else sizes(geo)
    for stream in NORESYNC:
        for size, tag in ((small, "8k"), (full, "64k")):
            for ending in NORESYNC_ENDINGS:
                t[f"noresync-{stream}-{tag}-{ending}"] = lambda a=stream, b=size, c=ending: noresync(geo, a, b, c)
    for name in NONE_CHAIN:
        t[name] = lambda name=name: none_chain(geo, name)
    for d in range(1, 30):
        t[f"straddle30-d{d}"] = lambda d=d: straddle(geo, 30, d)
    for d in range(1, 13):
        t[f"straddle13-d{d}"] = lambda d=d: straddle(geo, 13, d)
    for rel, tag in ((-1, "m1"), (0, "0"), (1, "p1")):
        t[f"pair-on-boundary-55-{tag}"] = lambda rel=rel: pair_on_boundary(geo, 5, 5, rel)
    t["pair-on-boundary-57-0"] = lambda: pair_on_boundary(geo, 5, 7, 0)
    for where, tag in ((-30, "m30"), (-1, "m1"), (0, "0"), (1, "p1"), ("last", "last")):
        t[f"eos-at-{tag}"] = lambda where=where: eos_at(geo, where)
    for last in (1, 8, 9):
        for ending in ("valid", "ones8", "zero", "padonly"):
            t[f"last-piece-{last}-{ending}"] = lambda a=last, b=ending: last_piece(geo, a, b)
    t["terminal-early"] = lambda: terminal_early(geo)
    for pb in (511, 512):
        t[f"ov-pb{pb}"] = lambda pb=pb: ov_case(geo, pb)
    for kind in ("exact", "plus1", "full_then_small", "list_plus1"):
        t[f"share-{kind}"] = lambda kind=kind: share(geo, kind)
    for which in CAPACITIES:
        t[f"huge-capacity-{which}"] = lambda which=which: capacity(geo, geo.huge_min, which)
    t["long-sweep"] = lambda: long_sweep(geo)
    t["long-ring"] = lambda: long_ring(geo)
    t["long-short-output"] = lambda: long_short_output(geo)
    t["long-tail"] = lambda: long_tail(geo)
    for count in CLAIM_COUNTS:
        t[f"long-claims-dense-{count}"] = lambda count=count: long_claims(geo, count, False, cus)
        t[f"long-claims-sprinkled-{count}"] = lambda count=count: long_claims(geo, count, True, cus)
    for nb in (200, 4000):
        for which in CAPACITIES:
            t[f"long-capacity-{nb}-{which}"] = lambda a=nb, b=which: capacity(geo, a, b)
    for which in NEIGHBOURS:
        for mod in (1, 15):
            t[f"neighbour-bytes-{which}-{mod}"] = lambda a=which, b=mod: neighbour(geo, a, b)
    return t


CASE_NAMES = tuple(_case_table(None, 0))  # (the names do not depend on the geometry)
HUGE_SINGLE = tuple(n for n in CASE_NAMES if n.split("-")[0] in ("noresync", "none", "straddle30", "straddle13", "pair",
                                                                 "eos", "last", "terminal", "ov"))


def names(prefix):
    return [n for n in CASE_NAMES if n.startswith(prefix)]


@functools.lru_cache(maxsize=None)
def case(name, cus=CUS_MAX):
    """The named case (kept: the cases are shared between tests and never modified). `cus` matters to
    long-claims only."""
    return _case_table(geometry("wave"), cus)[name]()


def layout(c):
    """(blob u8, in_off i64 [n+1], out_off i64 [n+1]) of a case"""
    lens = np.fromiter((len(x) for x in c.lits), np.int64, len(c.lits))
    io = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=io[1:])
    caps = lens * 8 // 5 if c.caps is None else np.asarray(c.caps, np.int64)
    oo = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(caps, out=oo[1:])
    return np.frombuffer(b"".join(c.lits), np.uint8).copy(), io, oo


def write_emu_file(path, lits):
    """the literals as `emu --file` reads them: u32 count, then per literal u32 bytes and the bytes"""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(lits)))
        for x in lits:
            f.write(struct.pack("<I", len(x)))
            f.write(x)


def gather(buf, starts, lens):
    """buf[starts[i] : starts[i] + lens[i]] laid end to end"""
    lens = np.asarray(lens, np.int64)
    tot = int(lens.sum())
    if tot == 0:
        return np.zeros(0, np.uint8)
    ends = np.cumsum(lens)
    idx = np.repeat(np.asarray(starts, np.int64)[: len(lens)] - (ends - lens), lens) + np.arange(tot)
    return buf[idx]


Expected = collections.namedtuple("Expected", "blob in_off out_off out_len status flat")


def expected(c):
    """The oracle's answer to a case: its status and decoded length per literal, or, where a literal's capacity is
    below its decoded size, HPK_OUTPUT_OVERFLOW (4) with out_len = the capacity; flat = every literal's first
    out_len decoded bytes end to end. One oracle call, on the case's distinct literals (the oracle builds a fresh
    decoder per literal, as the reference does: 10 us each, and the claim batches repeat a small pool of literals
    several hundred thousand times)."""
    from hpk_util import oracle_decode_batch, pack

    blob, io, oo = layout(c)
    first = {}
    inv = np.fromiter((first.setdefault(x, len(first)) for x in c.lits), np.int64, len(c.lits))
    ob, obo, ol, st = oracle_decode_batch(*pack(list(first)))
    ol, caps = ol.astype(np.int64)[inv], np.diff(oo)
    status = np.where(ol > caps, 4, st[inv]).astype(np.uint8)
    out_len = np.minimum(ol, caps)
    return Expected(blob, io, oo, out_len, status, gather(ob, obo.astype(np.int64)[inv], out_len))


@functools.lru_cache(maxsize=None)
def expected_of(name, cus=CUS_MAX):
    return expected(case(name, cus))
