"""The header-block plan's reference model and its placed cases (hpk_plan_blocks, loona_amd/csrc/hpk_blkplan.h).

ref_plan is a Python model of the call: per encoder a table of (name, value) entries, newest first
(blocks_apply_cases.Table), the encoder's blocks in order, a block a list of (name, value), and whether the encoder
Huffman-codes. Per header it gives the kind, the index, the prefix octets and the three items (policy, bytes) that
hpk_pack_batch and hpk_encode_strings_packed would be handed; per encoder the blocks planned and the final table,
with the call's deferral rule for a given ring size. Names and values are bytes here, where the library moves
references into an arena; the tests resolve the library's references before they compare.
tests/test_blocks_plan_cases.py pins ref_plan to hpack_ref.Encoder; the emulation and the GPU tests compare the real
code with it."""

import random

import numpy as np

import blocks_apply_cases as ac
import blocks_scan_cases as bc
from hpk_util import hpack_ref

NONE, INDEXED, NAME_INDEXED, NEW_NAME = 0, 1, 2, 3  # hpk_plan_kind
AUTO, RAW, VERBATIM = 0, 1, 3  # the policies the plan hands out (hpk.h HPK_STR_*)
EMPTY = (VERBATIM, b"")
DEFAULT = (NONE, 0, b"", [EMPTY, EMPTY, EMPTY])  # a header nobody planned

Table = ac.Table
entry = ac.entry


def find_header(tab, static, name, value):
    """HeaderTable::find_header (lib.rs:261-288) -> (the lowest index that matches whole or 0, the highest index
    whose name matches or 0); 1-based, the static entries first, then the table, newest first"""
    last = 0
    for i, (n, v) in enumerate(static):
        if n == name:
            if v == value:
                return i + 1, last
            last = i + 1
    for i, (n, v) in enumerate(tab.entries):
        if n == name:
            if v == value:
                return len(static) + 1 + i, last
            last = len(static) + 1 + i
    return 0, last


def plan_header(tab, static, name, value, policy):
    """Encoder::encode's body for one header (encoder.rs:246-264) -> (kind, index, prefix, items); the table changed"""
    full, last = find_header(tab, static, name, value)
    if full:
        p = hpack_ref.encode_integer(full, 7, 0x80)
        return INDEXED, full, p, [(VERBATIM, p), EMPTY, EMPTY]
    if last:
        p = hpack_ref.encode_integer(last, 4, 0x00)
        return NAME_INDEXED, last, p, [(VERBATIM, p), (policy, value), EMPTY]
    tab.insert(name, value)
    return NEW_NAME, 0, b"\x40", [(VERBATIM, b"\x40"), (policy, name), (policy, value)]


def ref_plan(encoders, ring):
    """encoders: [(Table, [block], huffman)], a block a list of (name, value). Plans each encoder's blocks in order,
    the tables changed in place -> [(results, planned)] per encoder: results one list of plan_header tuples per
    block, or None per block of an encoder that is deferred (the ring could not hold its table at the call's start)"""
    static = ac.static_table()
    out = []
    for tab, blocks, huffman in encoders:
        lim = ring if tab.cap is None else min(ring, tab.cap)
        if tab.max_size > 32 * lim or len(tab.entries) > lim:
            out.append(([None] * len(blocks), 0))
            continue
        pol = AUTO if huffman else RAW
        out.append(([[plan_header(tab, static, bytes(n), bytes(v), pol) for n, v in blk] for blk in blocks], len(blocks)))
    return out


def assemble(blocks_items):
    """[[items of a header] per block ...] -> the blocks' bytes: every item through encode_strings_cases.expected, the
    answer of hpk_encode_strings_packed, in one call; a block is its headers' items end to end"""
    import encode_strings_cases as sc

    flat = [it for blk in blocks_items for items in blk for it in items]
    x = sc.expected([s for _, s in flat], np.array([p for p, _ in flat], np.uint8))
    cuts = np.concatenate([[0], np.cumsum([3 * len(blk) for blk in blocks_items])]).astype(np.int64)
    at = x.out_off[cuts]
    return [x.flat[int(a) : int(b)].tobytes() for a, b in zip(at[:-1], at[1:])]


# ---- placed cases ----------------------------------------------------------------------------------------------
_collisions = {}


def collisions(seed=7541, cap=1 << 19):
    """-> (a, b), (c, d): two pairs of different 8-byte strings with equal hash under the kernel's hash
    (hpk_test_blkplan_hash), by a seeded birthday search over at most 2^19 candidates: with 32 bits of hash some
    thirty pairs are expected among them. It must find both pairs."""
    if seed not in _collisions:
        from loona_amd import _lib

        rng = np.random.default_rng(seed)
        alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789-", np.uint8)
        blob = np.ascontiguousarray(alpha[rng.integers(0, len(alpha), (cap, 8))])
        off = (np.arange(cap + 1, dtype=np.uint32) * 8).astype(np.uint32)
        out = np.zeros(cap, np.uint32)
        assert _lib.lib().hpk_test_blkplan_hash(blob.ctypes.data, off.ctypes.data, cap, out.ctypes.data) == _lib.HPK_E_OK
        order = np.argsort(out, kind="stable")
        same = np.nonzero(out[order][1:] == out[order][:-1])[0]
        pairs = []
        for k in same:
            a, b = blob[order[k]].tobytes(), blob[order[k + 1]].tobytes()
            if a != b and all(a not in p and b not in p for p in pairs):
                pairs.append((a, b))
            if len(pairs) == 2:
                break
        assert len(pairs) == 2, "the birthday search found %d colliding pairs" % len(pairs)
        _collisions[seed] = tuple(pairs)
    return _collisions[seed]


def fillers(n, first=1000):
    """n entries of 40 octets with names no case asks for"""
    return [(b"f%04d" % (first + k), b"val") for k in range(n)]


def placed(ring=2048, chunk=64, group=64):
    """[(name, Table, [block], huffman, expect)]: one encoder each. expect, written by hand from RFC 7541 and
    encoder.rs: "wire", the blocks' bytes (raw string literals); "reps", {(block, position): (kind, index)}; and
    optional "count" / "size" / "max_size" / "planned" of the end state. The cases lie relative to the kernel's
    geometry: its ring's records, the headers a wave stages at a time and the entries a search step tests."""
    out = []

    def add(name, tab, blocks, huffman=False, **expect):
        out.append((name, tab, [[(bytes(n), bytes(v)) for n, v in b] for b in blocks], huffman, expect))

    raw = ac.raw
    get = (b":method", b"GET")
    add("a static full match", Table(), [[get]], wire=[b"\x82"], count=0)
    add("a static last-name match", Table(), [[(b":method", b"PUT"), (b":status", b"999")]],
        wire=[b"\x03\x03PUT\x0e\x03999"], reps={(0, 0): (NAME_INDEXED, 3), (0, 1): (NAME_INDEXED, 14)}, count=0)
    add("an empty value that matches a static entry whole", Table(), [[(b"accept-charset", b"")]], wire=[b"\x8f"])
    add("an empty name and an empty value", Table(), [[(b"", b"")]], wire=[b"\x40\x00\x00"], count=1, size=32)
    add("the same new header twice in one chunk", Table(), [[(b"x-a", b"1"), (b"x-a", b"1")]], wire=[b"\x40\x03x-a\x011\xbe"],
        count=1)
    add("the same new header at a chunk's last and the next chunk's first position", Table(),
        [[get] * (chunk - 1) + [(b"x-b", b"2")] * 2], reps={(0, chunk - 1): (NEW_NAME, 0), (0, chunk): (INDEXED, 62)}, count=1)
    add("carried-in entries of one name: the highest index", Table([(b"n", b"a"), (b"n", b"b"), (b"n", b"c")]), [[(b"n", b"z")]],
        wire=[b"\x0f\x31\x01z"], reps={(0, 0): (NAME_INDEXED, 64)}, count=3)
    add("carried-in duplicates: the lowest index", Table([(b"n", b"a"), (b"n", b"a")]), [[(b"n", b"a")]], wire=[b"\xbe"], count=2)
    add("a dynamic full match against a static name match", Table([(b":method", b"PUT")]), [[(b":method", b"PUT")]], wire=[b"\xbe"])
    add("a dynamic name match above the static ones", Table([(b":method", b"X")]), [[(b":method", b"Y")]], wire=[b"\x0f\x2f\x01Y"],
        reps={(0, 0): (NAME_INDEXED, 62)})
    # the search's groups: group 0 is the static entries, group g >= 1 the table's entries 64 (g - 1) .. 64 g - 1
    big = 1 << 15
    for p in (group - 1, group, group + 1):
        ents = fillers(3 * group + 2)
        ents[5] = (b"srch", b"other")
        ents[p] = (b"srch", b"it")
        add(f"a full match at search position {p} behind a name match in the first group", Table(ents, big), [[(b"srch", b"it")]],
            reps={(0, 0): (INDEXED, 62 + p)})
        ents = fillers(3 * group + 2)
        ents[5] = (b"srch", b"a")
        ents[p + group] = (b"srch", b"b")
        add(f"name matches in the first group and at position {p + group}", Table(ents, big), [[(b"srch", b"it")]],
            reps={(0, 0): (NAME_INDEXED, 62 + p + group)})
        ents = fillers(3 * group + 2)
        ents[3] = ents[p] = (b"srch", b"it")
        add(f"full matches in the first group and at position {p}", Table(ents, big), [[(b"srch", b"it")]], reps={(0, 0): (INDEXED, 65)})
        ents = fillers(3 * group + 2)
        ents[p] = ents[p + group] = (b"srch", b"it")
        ents[p + 1] = (b"srch", b"later")
        add(f"full matches at positions {p} and {p + group}", Table(ents, big), [[(b"srch", b"it")]], reps={(0, 0): (INDEXED, 62 + p)})
    # equal hashes, different bytes
    (na, nb), (va, vb) = collisions()
    add("two names of equal hash", Table([(na, b"1")]), [[(nb, b"2")]], wire=[b"\x40" + raw(nb) + raw(b"2")], count=2)
    add("two values of equal hash under one name", Table([(b"nm", va)]), [[(b"nm", vb)]], wire=[b"\x0f\x2f" + raw(vb)], count=1)
    add("a name whose hash an entry with the same value has", Table([(na, b"same")]), [[(nb, b"same")]],
        wire=[b"\x40" + raw(nb) + raw(b"same")], count=2)
    add("a name and a value of equal hashes, the other way round", Table([(nb, vb)]), [[(na, va), (nb, va), (nb, vb)]],
        reps={(0, 0): (NEW_NAME, 0), (0, 1): (NAME_INDEXED, 63), (0, 2): (INDEXED, 63)}, count=2)
    add("a name that is a proper prefix of an entry's", Table([(b"x-long-name", b"v")]), [[(b"x-long", b"v"), (b"accep", b"")]],
        reps={(0, 0): (NEW_NAME, 0), (0, 1): (NEW_NAME, 0)}, count=3)
    # eviction by insertion
    add("an insertion that fits exactly", Table([entry(0)], max_size=80), [[entry(1)]], wire=[b"\x40" + raw(entry(1)[0]) + raw(entry(1)[1])],
        count=2, size=80)
    add("an insertion that evicts the one entry", Table([entry(0)], max_size=79), [[entry(1), entry(0)]],
        reps={(0, 0): (NEW_NAME, 0), (0, 1): (NEW_NAME, 0)}, count=1, size=40)
    e41 = entry(1, 41)
    add("an entry above max_size empties the table and is still a new name", Table([entry(0)], max_size=40), [[e41, entry(0)]],
        wire=[b"\x40" + raw(e41[0]) + raw(e41[1]) + b"\x40" + raw(entry(0)[0]) + raw(entry(0)[1])], count=1, size=40)
    add("max_size 0", Table(max_size=0), [[(b"a", b"b"), (b"a", b"b")]], wire=[b"\x40\x01a\x01b" * 2], count=0, size=0, max_size=0)
    # more insertions than the ring has records: the ring's head wraps, 64 entries of 64 octets live
    per = 16
    nblk = (ring + 2 * chunk) // per + 1
    wrap = [[entry(b * per + i, 64) for i in range(per)] + ([entry((b - 3) * per, 64)] if b >= 3 else []) for b in range(nblk)]
    add("more insertions than the ring's records", Table(), wrap,
        reps={(b, per): (INDEXED, 61 + 64) for b in range(3, nblk)}, count=64, size=4096)
    # index octet counts
    ents = fillers(100)
    add("7-bit-prefix indices 126, 127, 128", Table(ents, big), [[ents[126 - 62], ents[127 - 62], ents[128 - 62]]],
        wire=[b"\xfe\xff\x00\xff\x01"], count=100)
    add("4-bit-prefix indices 14, 15, 16", Table(), [[(b":status", b"1"), (b"accept-charset", b"2"), (b"accept-encoding", b"3")]],
        wire=[b"\x0e\x011\x0f\x00\x012\x0f\x01\x013"], count=0)
    names = [ents[k - 62][0] for k in (142, 143, 144)]
    add("4-bit-prefix indices 142, 143, 144", Table(ents, big), [[(n, b"q") for n in names]],
        wire=[b"\x0f\x7f\x01q\x0f\x80\x01\x01q\x0f\x81\x01\x01q"], count=100)
    add("index 61 + ring_entries from a table of minimal entries", Table([(b"", b"")] * ring, 32 * ring), [[(b"", b"x"), (b"", b"")]],
        wire=[hpack_ref.encode_integer(61 + ring, 4, 0) + b"\x01x\xbe"], reps={(0, 0): (NAME_INDEXED, 61 + ring), (0, 1): (INDEXED, 62)},
        count=ring, size=32 * ring)
    # block and list shapes
    mix = [get, (b":path", b"/x"), (b"x-n", b"1"), (b"x-n", b"2"), (b":status", b"200")]
    sizes = (1, 0, chunk - 1, chunk, chunk + 1, 2 * chunk + 1)
    later = [(INDEXED, 2), (NAME_INDEXED, 5), (INDEXED, 62), (NAME_INDEXED, 62), (INDEXED, 8)]  # once x-n: 1 is in the table
    reps = {(5, i): later[i % 5] for i in range(2 * chunk + 1)}
    reps.update({(0, 0): (INDEXED, 2), (2, 1): (NAME_INDEXED, 5), (2, 2): (NEW_NAME, 0), (2, 3): (NAME_INDEXED, 62), (2, 7): (INDEXED, 62)})
    add("blocks of 1, 0, 63, 64, 65 and 129 headers", Table(), [[mix[i % 5] for i in range(n)] for n in sizes], reps=reps, count=1,
        planned=len(sizes))
    add("an encoder with no blocks", Table(fillers(3)), [], count=3, planned=0)
    add("a list of 65 blocks", Table(), [[(b"x-%d" % (k // 2), b"v"), get] for k in range(65)],
        reps={(0, 0): (NEW_NAME, 0), (1, 0): (INDEXED, 62), (2, 0): (NEW_NAME, 0), (63, 0): (INDEXED, 62), (64, 0): (NEW_NAME, 0),
              (64, 1): (INDEXED, 2)}, count=33, planned=65)
    add("a Huffman-coding encoder", Table(), [[(b"x-huff", b"aaaaaaaaaaaaaaaa"), (b":path", b"/index.html")]], huffman=True,
        reps={(0, 0): (NEW_NAME, 0), (0, 1): (INDEXED, 5)}, count=1)
    # deferral
    add("max_size above 32 * lim at the start", Table(fillers(3), max_size=32 * ring + 1), [[get], [get]], count=3, max_size=32 * ring + 1,
        planned=0)
    add("max_size of exactly 32 * lim", Table(fillers(3), max_size=32 * ring), [[get]], wire=[b"\x82"], count=3, planned=1)
    add("count above lim at the start", Table([(b"", b"")] * (ring + 1), 32 * ring), [[get]], count=ring + 1, planned=0)
    add("cap below the ring's records: max_size above 32 * cap", Table(fillers(3), cap=8), [[get]], count=3, planned=0)
    add("cap below the ring's records: within 32 * cap", Table(fillers(3), max_size=256, cap=8), [[entry(9), get]],
        reps={(0, 0): (NEW_NAME, 0)}, count=4, size=160, planned=1)
    return out


def check_expect(name, tab, results, planned, expect):
    """the placed case's edge, on any result in ref_plan's form and the table after it"""
    if "planned" in expect:
        assert planned == expect["planned"], name
    if "wire" in expect:
        assert planned == len(results) and assemble([[items for _, _, _, items in blk] for blk in results]) == expect["wire"], name
    for (b, i), (kind, index) in expect.get("reps", {}).items():
        assert results[b][i][:2] == (kind, index), (name, b, i, results[b][i][:2])
    if "count" in expect:
        assert len(tab.entries) == expect["count"], (name, len(tab.entries))
    for key in ("size", "max_size"):
        if key in expect:
            assert getattr(tab, key) == expect[key], (name, key, getattr(tab, key))
    assert tab.size == sum(len(n) + len(v) + 32 for n, v in tab.entries) or planned == 0, name


# ---- corpora ---------------------------------------------------------------------------------------------------
def story_headers():
    """[[block]]: the interop stories' header lists, a list of blocks per story"""
    return [[[(n.encode(), v.encode()) for n, v in c["headers"]] for c in story["cases"]] for _, story in bc.stories()]


def random_lists(seed=61, n=300):
    """[[block]]: seeded header lists over a small vocabulary, so that names and whole headers repeat, static ones
    among them; one to four blocks per encoder"""
    rng = random.Random(seed)
    static = ac.static_table()
    names = [s[0] for s in static[::5]] + [b"x-%d" % k for k in range(12)] + [b"", b"x", b"x-"]
    values = [s[1] for s in static[::7]] + [b"v%d" % k for k in range(10)] + [b"", b"v", bytes(range(200, 232))]
    out = []
    for _ in range(n):
        out.append([[(rng.choice(names), rng.choice(values)) if rng.random() < 0.8 else rng.choice(static)
                     for _ in range(rng.randrange(0, 40))] for _ in range(rng.randrange(1, 5))])
    return out


def carried(ring=2048):
    """placed case 20, tables carried over two and three calls -> ([(blocks, huffman)], [Table]): twelve interop
    stories and twelve random lists of at least three blocks, with the tables their first call starts from (small
    limits among them, so that what is carried was shaped by evictions). A test cuts every encoder's blocks into the
    calls' parts and feeds each call the tables the call before left."""
    c = corpora(ring)
    stories = [(blocks, h) for _, blocks, h in c["interop"][:: 159 // 12][:12]]
    stories += [(blocks, h) for _, blocks, h in c["random"] if len(blocks) >= 3][:12]
    return stories, [Table(max_size=(4096, 512, 100)[k % 3]) for k in range(len(stories))]


_corpora = {}


def corpora(ring=2048, chunk=64, group=64):
    """{name: [(Table, [block], huffman)]}: the encoders every check of the plan runs over (built once; copy a Table
    before planning against it): the interop stories' header lists, the random lists with small and default tables,
    and the placed cases"""
    key = (ring, chunk, group)
    if key not in _corpora:
        c = {}
        c["interop"] = [(Table(), blocks, k % 2 == 1) for k, blocks in enumerate(story_headers())]
        c["random"] = [(Table(max_size=(4096, 256, 100, 0)[k % 4]), blocks, k % 3 == 0) for k, blocks in enumerate(random_lists())]
        c["placed"] = [(tab, blocks, huffman) for _, tab, blocks, huffman, _ in placed(ring, chunk, group)]
        _corpora[key] = c
    return _corpora[key]


def fresh(encoders):
    return [(tab.copy(), blocks, huffman) for tab, blocks, huffman in encoders]
