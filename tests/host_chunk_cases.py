"""Placed cases for the host-pointer batches (hpk_decode_batch / hpk_encode_batch with HPK_PTR_HOST), which
loona_amd/csrc/hpk_calls_batch.hip cuts into up to 8 literal ranges ("chunks") by the arithmetic of hpk_chunks.h: the
copy-in, the kernel and the copy-out of neighbouring chunks overlap on three streams, over shared staging buffers
and absolute offsets. Shared by test_host_chunk_cases.py (CPU: the model below against the replay of the real
header, tests/emu/chunks_emu.cpp, and every case reaching the edge it is named for) and test_gpu_host_chunks.py
(every case through the host form against the C oracle, bit for bit).

cuts() is a model of the cut arithmetic written from the pipeline's description: one chunk per 4 MiB of input
and output bytes together, at least 1, at most 8, at most one per literal; cut[j] is the first literal whose end
(its absolute in_off) is at or past floor(in_off[n] * j / chunks). It looks at every literal in turn; the header
searches by halving.

A case is Case(kind, lits, in_off, out_off, in_cap, out_cap, meta): kind "decode" (lits are Huffman literals) or
"encode" (lits are the plain strings), the offsets as the caller passes them (int64 arrays of n + 1 entries), the
bytes the caller's two blobs hold, and what the case claims about itself. The cases are small in literals and
large only in declared output capacity: the chunk count follows in_off[n] + out_off[n], so a few dozen literals
whose regions span 32 MiB are cut into 8 chunks, and since the cuts go by encoded bytes, literals of chosen
lengths place every cut exactly. Regions without a capacity of their own share the span evenly (an odd number of
bytes each, so region starts take every alignment); a region with a capacity of its own has exactly that.

expected() takes a case's answer from the C oracle by the rule of decode_long_cases.expected: the oracle's status
and length, or, where a region is shorter than the result, status 4 with out_len = the capacity and the result's
first out_len bytes (include/hpk.h; for the encode: "out_len = the capacity, holding the encoding's prefix")."""

import collections
import functools

import numpy as np

from decode_long_cases import BAD_PADS, BITS, LEN, Stream, _seed, gather, long_stream, valid

MAX_CHUNKS = 8  # kHpkMaxChunks (checked against the header by test_host_chunk_cases.py)
CHUNK_BYTES = 4 << 20  # kHpkChunkBytes
HPK_MAX_OFFSET = 0xFFFFFFDF

Case = collections.namedtuple("Case", "kind lits in_off out_off in_cap out_cap meta")
Expected = collections.namedtuple("Expected", "out_len status flat")


# ---- the model ---------------------------------------------------------------------------------------------------

def chunk_count(in_bytes, out_bytes, n):
    return min(max((in_bytes + out_bytes) // CHUNK_BYTES, 1), MAX_CHUNKS, n)


def cuts_of(in_off, out_bytes):
    """(chunks, [cut[0], ..., cut[chunks]]) of a batch with these input offsets and out_off[n] = out_bytes"""
    ends = np.asarray(in_off, np.int64)[1:]
    n = len(ends)
    in_bytes = int(in_off[-1])
    chunks = chunk_count(in_bytes, int(out_bytes), n)
    cut = [0]
    for j in range(1, chunks):
        passed = np.nonzero(ends >= in_bytes * j // chunks)[0]
        cut.append(int(passed[0]) if passed.size else n)
    if chunks:
        cut.append(n)
    return chunks, cut


def cuts(in_off, out_off):
    return cuts_of(in_off, int(out_off[-1]))


def targets(c):
    """the byte position cut j = 1 .. chunks - 1 aims at"""
    chunks, _ = cuts(c.in_off, c.out_off)
    return [int(c.in_off[-1]) * j // chunks for j in range(1, chunks)]


# ---- building blocks -----------------------------------------------------------------------------------------------

TEXT = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789-_=;,/.:ABCXYZ %&*\"", np.uint8)
ERRORS = {"ptl": 1, "ip": 2, "eos": 3, "short": 4}  # PaddingTooLarge, InvalidPadding, EOSInString, a capacity one short


def encoded_len(raw):
    return (sum(LEN[b] for b in raw) + 7) // 8


def literal(what, nbytes, rng):
    """(a literal of exactly nbytes, the symbols a decoder gets from it): valid text, or text that ends in eight
    ones, in a zero among the padding bits, or that meets EOS after 41 bits (random bytes behind it)"""
    s, tot = Stream(rng), 8 * nbytes
    if what in ("ok", "short"):
        s.finish(nbytes)
    elif what == "ptl":
        s.fill_to(tot - 8).raw("1" * 8)
    elif what == "ip":
        s.fill_to(tot - 4).raw(BAD_PADS[4])
    else:
        assert what == "eos"
        s.fill_to(41).eos().random_to(nbytes)
    return s.bytes(), s.count


def place(kind, lits, caps=None, chunks=MAX_CHUNKS, slack="spread", in_base=0, out_base=0, gap=0, meta=None):
    """The case of these literals. caps[i]: literal i's region, None for its bound plus a share of the bytes that
    bring in_off[n] + out_off[n] to `chunks` chunks' worth (slack = "spread"), or all of them on region `slack`.
    gap: bytes the caller's blobs have behind the last region."""
    n = len(lits)
    lens = np.fromiter((len(x) for x in lits), np.int64, n)
    in_off = np.full(n + 1, in_base, np.int64)
    in_off[1:] += np.cumsum(lens)
    caps = [None] * n if caps is None else list(caps)
    own = 8 * lens // 5 if kind == "decode" else (30 * lens + 7) // 8
    free = np.array([c is None for c in caps], bool)
    region = np.where(free, own, np.array([0 if c is None else c for c in caps], np.int64))
    need = chunks * CHUNK_BYTES - int(in_off[n]) - out_base - int(region.sum())
    if need > 0 and slack == "spread":
        assert free.any()
        region[free] += -(-need // int(free.sum())) | 1
    elif need > 0:
        assert free[slack]
        region[slack] += need
    out_off = np.full(n + 1, out_base, np.int64)
    out_off[1:] += np.cumsum(region)
    assert cuts(in_off, out_off)[0] == min(chunks, n) and out_off[n] <= HPK_MAX_OFFSET
    return Case(kind, list(lits), in_off, out_off, int(in_off[n]) + gap, int(out_off[n]) + gap, dict(meta or {}))


def in_blob(c, junk=0xEE):
    """the caller's input blob: the literals at their offsets, `junk` before in_off[0] and behind in_off[n]"""
    b = np.full(max(c.in_cap, 1), junk, np.uint8)
    data = np.frombuffer(b"".join(c.lits), np.uint8)
    b[int(c.in_off[0]) : int(c.in_off[0]) + data.size] = data
    return b


def base24(rng, nbytes=40):
    """24 valid literals of 40 bytes: 8 chunks, cut[j] = 3 j - 1 (literal 3 j - 1 ends on j/8 of the bytes)"""
    return [valid(nbytes, rng) for _ in range(24)]


# ---- the cases -----------------------------------------------------------------------------------------------------

def collapsed(where):
    """one literal with more than 7/8 of the encoded bytes (a long one, in the middle a huge one) among 16 of 10
    bytes: every cut is that literal, and the chunks between the first and the last are empty"""
    rng = _seed(f"collapsed-{where}")
    small = [valid(10, rng) for _ in range(16)]
    at = {"first": 0, "middle": 8, "last": 16}[where]
    big = valid(9000 if where == "middle" else 4000, rng)
    return place("decode", small[:at] + [big] + small[at:], meta={"big": at})


def no_input():
    return place("decode", [b""] * 20)


def few(n):
    rng = _seed(f"few-{n}")
    return place("decode", [valid(40, rng) for _ in range(n)])


def target(how):
    """literal 3 j - 1 ends exactly on cut j's target, one byte before it, or one byte after it (j = 1 .. 7)"""
    rng = _seed(f"target-{how}")
    d = {"on": 0, "before": -1, "after": 1}[how]
    lens = [40] * 24
    for j in range(1, 8):
        lens[3 * j - 1] += d
        lens[3 * j] -= d
    return place("decode", [valid(x, rng) for x in lens], meta={"d": d})


def empties_on_cut():
    """per chunk: two literals, three empty ones, the literal X that takes the cut, three empty ones. X ends one
    byte past the target behind the even groups and exactly on it behind the odd ones"""
    rng = _seed("empties-on-cut")
    lits, takers = [], []
    for g in range(8):
        a, b, x = (40, 40, 41) if g % 2 == 0 else (40, 39, 40)
        lits += [valid(a, rng), valid(b, rng), b"", b"", b""]
        takers.append(len(lits))
        lits += [valid(x, rng), b"", b"", b""]
    return place("decode", lits, meta={"takers": takers})


def align(shift):
    """groups of 64, 32 and 32 bytes behind a leading literal of `shift` bytes (an empty one for 0): the literal that
    takes cut j starts at byte 128 j - 32 + shift, so every cut lies at `shift` mod 16. The groups are the same
    literals whatever the shift."""
    rng = _seed("align")
    groups = [valid(nb, rng) for _ in range(8) for nb in (64, 32, 32)]
    lead = valid(shift, _seed(f"align-lead-{shift}")) if shift else b""
    return place("decode", [lead] + groups, meta={"shift": shift})


def seam_error(what, side):
    """the first (or the last) literal of every chunk is an error literal of this kind, all others are valid"""
    rng = _seed(f"seam-{what}-{side}")
    lits, caps, rows = base24(rng), [None] * 24, []
    _, cut = cuts_of(np.arange(25) * 40, MAX_CHUNKS * CHUNK_BYTES)
    for j in range(MAX_CHUNKS):
        i = cut[j] if side == "first" else cut[j + 1] - 1
        lits[i], count = literal(what, 40, rng)
        if what == "short":
            caps[i] = count - 1
        rows.append(i)
    return place("decode", lits, caps, meta={"rows": rows, "status": ERRORS[what]})


SEAM_SIZES = (63, 64, 65, 8191, 8192, 8193)


def seam_size(nbytes):
    """two literals of nbytes (text, then 5-bit codes that fill the decoded bound) with a cut between them: the
    literals behind them hold two bytes more than those in front, so half of the bytes ends inside the second"""
    rng = _seed(f"seam-size-{nbytes}")
    k, s = (6, 32) if nbytes < 1000 else (12, 40)
    pre = [valid(s, rng) for _ in range(k)]
    post = [valid(s, rng) for _ in range(k - 1)] + [valid(s + 2, rng)]
    return place("decode", pre + [valid(nbytes, rng), long_stream("five", nbytes, rng)[0]] + post, meta={"first_big": k})


def dense_long():
    """two chunks: twelve long literals (100 to 199 bytes), then sixty of 30 bytes"""
    rng = _seed("dense-long")
    longs = [valid(100 + 9 * i, rng) for i in range(12)]
    return place("decode", longs + [valid(30, rng) for _ in range(60)], chunks=2, meta={"longs": 12})


def exact_regions():
    """24 literals of 41 bytes of 5-bit codes: each decodes to its bound of 65 bytes, its region is exactly that,
    and the regions stand back to back (the bytes that make 8 chunks are the last region's)"""
    rng = _seed("exact-regions")
    lits = [long_stream("five", 41, rng)[0] for _ in range(24)]
    return place("decode", lits, [65] * 23 + [None], slack=23)


def encode_exact(short):
    """the encode twin: 24 strings of 40 bytes, each region exactly its encoded length, back to back; short: the
    regions on both sides of cuts 3 and 5 are one byte short"""
    rng = _seed("encode-exact")
    raws = [rng.choice(TEXT, 40).tobytes() for _ in range(24)]
    caps = [encoded_len(x) for x in raws[:23]] + [None]
    rows = [8 - 1, 8, 14 - 1, 14] if short else []  # cut[j] = 3 j - 1
    for i in rows:
        caps[i] -= 1
    return place("encode", raws, caps, slack=23, meta={"rows": rows})


def encode_text():
    """48 strings of 1 to 120 bytes (text, and every eighth of any bytes) into bound-sized regions"""
    rng = _seed("encode-text")
    raws = [(rng.integers(0, 256, int(rng.integers(1, 121)), dtype=np.uint8) if i % 8 == 7 else
             rng.choice(TEXT, int(rng.integers(1, 121)))).tobytes() for i in range(48)]
    return place("encode", raws)


def bases(kind):
    """in_off[0] = 5 and out_off[0] = 7, and 37 bytes of both blobs behind the last region"""
    rng = _seed(f"bases-{kind}")
    lits = base24(rng) if kind == "decode" else [rng.choice(TEXT, 40).tobytes() for _ in range(24)]
    return place(kind, lits, in_base=5, out_base=7, gap=37)


def small3():
    """three literals, one chunk: the small call of the over-time tests"""
    rng = _seed("small3")
    return place("decode", [valid(11, rng), valid(70, rng), valid(5, rng)], chunks=1)


def _table():
    t = {}
    for where in ("first", "middle", "last"):
        t[f"collapsed-{where}"] = lambda where=where: collapsed(where)
    t["no-input"] = no_input
    for n in (1, 3, 7):
        t[f"few-{n}"] = lambda n=n: few(n)
    for how in ("on", "before", "after"):
        t[f"target-{how}"] = lambda how=how: target(how)
    t["empties-on-cut"] = empties_on_cut
    for shift in (0, 1, 15):
        t[f"align-{shift}"] = lambda shift=shift: align(shift)
    for what in ERRORS:
        for side in ("first", "last"):
            t[f"seam-{what}-{side}"] = lambda what=what, side=side: seam_error(what, side)
    for nb in SEAM_SIZES:
        t[f"seam-size-{nb}"] = lambda nb=nb: seam_size(nb)
    t["dense-long"] = dense_long
    t["exact-regions"] = exact_regions
    t["bases-decode"] = lambda: bases("decode")
    t["small3"] = small3
    t["encode-exact"] = lambda: encode_exact(False)
    t["encode-short"] = lambda: encode_exact(True)
    t["encode-text"] = encode_text
    t["bases-encode"] = lambda: bases("encode")
    return t


_TABLE = _table()
CASE_NAMES = tuple(_TABLE)
DECODE_NAMES = tuple(n for n in CASE_NAMES if not n.startswith("encode") and n != "bases-encode")
ENCODE_NAMES = tuple(n for n in CASE_NAMES if n not in DECODE_NAMES)


@functools.lru_cache(maxsize=None)
def case(name):
    """The named case (kept: the cases are shared between tests and never modified)."""
    return _TABLE[name]()


def expected(c):
    from hpk_util import oracle_decode_batch, oracle_encode_batch, pack

    first = {}
    inv = np.fromiter((first.setdefault(x, len(first)) for x in c.lits), np.int64, len(c.lits))
    ob, obo, ol, st = (oracle_decode_batch if c.kind == "decode" else oracle_encode_batch)(*pack(list(first)))
    ol, caps = ol.astype(np.int64)[inv], np.diff(c.out_off)
    status = np.where(ol > caps, 4, st[inv]).astype(np.uint8)
    out_len = np.minimum(ol, caps)
    return Expected(out_len, status, gather(ob, obo.astype(np.int64)[inv], out_len))


@functools.lru_cache(maxsize=None)
def expected_of(name):
    return expected(case(name))


# ---- the differential batch ----------------------------------------------------------------------------------------

DIFF_N = 60_000
DIFF_SEED = 20
ONE_ZERO = [s for s in range(256) if LEN[s] == 30 and BITS[s].count("0") == 1]  # one flip away from EOS


@functools.lru_cache(maxsize=2)
def differential(seed=DIFF_SEED, n=DIFF_N):
    """(case, expected): n literals with synth.config3's lengths and bytes, about 2 % of them cut short by 1 to 4
    bytes or with one bit flipped: any bit, or for a fifth of them the single zero of a 30-bit code that has only
    one, which makes it EOS (no flip of a bit drawn evenly met EOS in 1,200 literals); every region its decoded
    bound plus 0 to 3 bytes plus a fixed pad (0 where the bytes make 8 chunks already), every 97th a few bytes below
    what the oracle decodes"""
    from hpk_util import oracle_decode_batch, pack

    from loona_amd import synth

    w = synth.config3(n=n, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    off = w.enc_off.astype(np.int64)
    lits = [w.enc_blob[off[i] : off[i + 1]].tobytes() for i in range(n)]
    doff = w.dec_off.astype(np.int64)
    codelen = np.array(LEN[:256], np.int64)
    for i in np.nonzero(rng.random(n) < 0.02)[0]:
        x = bytearray(lits[i])
        how = rng.random()
        if how < 0.45:
            del x[max(1, len(x) - int(rng.integers(1, 5))) :]
        else:
            bit = int(rng.integers(0, 8 * len(x)))
            dec = w.dec_blob[doff[i] : doff[i + 1]]
            ones = np.nonzero(np.isin(dec, ONE_ZERO))[0]
            if how >= 0.8 and ones.size:  # the zero of the literal's first 30-bit code with a single zero: EOS
                k = int(ones[0])
                bit = int(codelen[dec[:k]].sum()) + BITS[int(dec[k])].index("0")
            x[bit // 8] ^= 0x80 >> bit % 8
        lits[i] = bytes(x)
    blob, io = pack(lits)
    _, _, ol, _ = oracle_decode_batch(blob, io)
    caps = 8 * np.diff(io.astype(np.int64)) // 5 + rng.integers(0, 4, n)
    cut_short = np.zeros(n, bool)
    for i in range(0, n, 97):
        if ol[i] > 0:
            caps[i], cut_short[i] = max(0, int(ol[i]) - 1 - i % 5), True
    need = MAX_CHUNKS * CHUNK_BYTES - int(io[-1]) - int(caps.sum())
    caps[~cut_short] += max(0, -(-need // int((~cut_short).sum())))
    c = place("decode", lits, [int(x) for x in caps])
    return c, expected(c)
