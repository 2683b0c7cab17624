"""The header-block apply on the GPU (hpk_apply_blocks through HuffmanCodec.apply_blocks), record for record: no
tolerance. Every call here is fed by the device's own scan_blocks and decode_strings, as a device-resident caller
would feed it; the arena (the static text, the carried-in entries' bytes, the packed strings) exists only on the
host, where the references that come back are resolved to bytes. The expected results are
blocks_apply_cases.ref_apply's (pinned to hpack_ref.Decoder by tests/test_blocks_apply_cases.py; the same corpora run
through the real step header on the CPU in tests/test_blkapply_emulation.py): per block the headers, the error and
its detail, per decoder the blocks applied and the final table entry by entry."""

import ctypes

import numpy as np
import pytest

import blocks_apply_cases as ac
import blocks_scan_cases as bc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 64  # sentinel bytes on both sides of every output array


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
    from loona_amd import _lib

    r, c, w = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    assert _lib.lib().hpk_test_blkapply_geometry(ctypes.byref(r), ctypes.byref(c), ctypes.byref(w)) == _lib.HPK_E_OK
    assert r.value >= 128 and r.value & (r.value - 1) == 0 and c.value == 64 and w.value >= 1
    return r.value, c.value


def i32(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.int64).astype(np.uint32)).view(np.int32)).cuda()


def guarded(nbytes, fill=0xA5):
    """a device byte buffer with GUARD sentinel bytes on both sides -> (whole, the nbytes in the middle)"""
    whole = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD : GUARD + nbytes]


def guards_intact(whole, fill=0xA5):
    h = whole.cpu().numpy()
    return bool((h[:GUARD] == fill).all() and (h[-GUARD:] == fill).all())


class Call:
    """one hpk_apply_blocks call over decoders [(Table, [block])], every piece kept so that a test can bend it"""

    def __init__(self, codec, decoders, ring, order="interleaved", unlisted=()):
        from loona_amd import batch

        self.codec, self.decoders, self.ring = codec, decoders, ring
        # the call's block list: the decoders' blocks interleaved (position by position), or decoder after decoder
        where = [(k, d) for d, (_, blocks) in enumerate(decoders) for k in range(len(blocks))]
        if order == "interleaved":
            where.sort()
        self.blocks = [decoders[d][1][k] for k, d in where] + list(unlisted)
        lists = [[] for _ in decoders]
        for b, (k, d) in enumerate(where):
            lists[d].append(b)
        self.lists = lists
        self.dec_blk = np.array([b for lst in lists for b in lst], dtype=np.uint32)
        self.dec_blk_off = np.concatenate([[0], np.cumsum([len(lst) for lst in lists])]).astype(np.uint32)
        self.blob = np.frombuffer(b"".join(self.blocks), dtype=np.uint8).copy()
        self.block_off = np.concatenate([[0], np.cumsum([len(w) for w in self.blocks])]).astype(np.uint32)
        # the arena: 16 bytes nobody refers to, the static text, the carried-in entries' bytes, the packed strings
        text, _ = batch.static_table()
        self.static_base = 16
        prior = b"".join(n + v for tab, _ in decoders for n, v in tab.entries)
        self.prior_base = self.static_base + len(text) + 5
        self.str_base = self.prior_base + len(prior) + 3
        self.arena_head = bytes(16) + text + bytes(5) + prior + bytes(3)
        tabs = np.zeros(len(decoders), dtype=batch.DTAB_DTYPE)
        ents = []
        at, e0 = self.prior_base, 0
        for d, (tab, _) in enumerate(decoders):
            cap = ring if tab.cap is None else tab.cap
            tabs[d] = (e0, cap, len(tab.entries), tab.size, tab.max_size,
                       0xFFFFFFFF if tab.max_allowed is None else tab.max_allowed, 0xDDDDDDDD, 0)
            rec = np.zeros(cap, dtype=batch.HEADER_DTYPE)
            for i, (n, v) in enumerate(tab.entries):
                rec[i] = (at, len(n), at + len(n), len(v))
                at += len(n) + len(v)
            ents.append(rec)
            e0 += cap
        self.tabs = tabs
        self.tab_ent = np.concatenate(ents) if ents else np.zeros(0, dtype=batch.HEADER_DTYPE)

    def scan(self, void_blocks=False):
        """the device's scan and string decode; everything stays on the device. void_blocks: the scan is to find
        bad block offsets (its sticky flag is read here, before the next call would report it)"""
        from loona_amd import _lib

        c = self.codec
        blob = torch.from_numpy(self.blob if self.blob.size else np.zeros(1, np.uint8)).cuda()[: self.blob.size]
        self.fields, self.field_off, so, se, sbo, _ = c.scan_blocks(blob, i32(self.block_off), sync=False)
        assert _lib.lib().hpk_ctx_check(c._h) == (_lib.HPK_E_INVAL if void_blocks else _lib.HPK_E_OK)
        totals = torch.stack([self.field_off[-1], sbo[-1]]).cpu().numpy().view(np.uint32)
        self.nf, self.ns = int(totals[0]), int(totals[1])
        self.packed, self.out_off, self.out_len, _, self.status = c.decode_strings(blob, so[: self.ns], se[: self.ns], sync=True)
        self.fields = self.fields[: 16 * self.nf]
        return self

    def apply(self, sync=True, headers_cap=None, nstrs=None, **bent):
        """-> the return of apply_blocks; the outputs are kept as device tensors with guards around them"""
        from loona_amd import batch

        c = self.codec
        hcap = self.nf if headers_cap is None else headers_cap
        self.g_headers, headers = guarded(16 * hcap)
        self.g_results, results = guarded(16 * len(self.blocks))
        self.g_tabs, tabs = guarded(32 * len(self.decoders))
        self.g_ent, ent = guarded(16 * len(self.tab_ent))
        self.used_tabs = bent.get("tabs", self.tabs)
        tabs.copy_(torch.from_numpy(self.used_tabs.view(np.uint8)).cuda())
        ent.copy_(torch.from_numpy(self.tab_ent.view(np.uint8)).cuda())
        self.d_tabs, self.d_ent, self.d_headers, self.d_results = tabs, ent, headers, results
        return c.apply_blocks(self.fields, bent.get("field_off", self.field_off), self.out_off, self.out_len, self.status,
                              self.ns if nstrs is None else nstrs, self.str_base, self.static_base,
                              i32(bent.get("dec_blk_off", self.dec_blk_off)), i32(bent.get("dec_blk", self.dec_blk)), tabs, ent,
                              headers=headers, results=results, sync=sync)

    def fetch(self, void=()):
        """the outputs on the host, every reference resolved against the arena -> [(results, applied, Table)]; for
        a decoder in `void` (its hpk_dtab was bent) the raw hpk_dtab record instead of the Table"""
        from loona_amd import batch

        assert all(guards_intact(g) for g in (self.g_headers, self.g_results, self.g_tabs, self.g_ent))
        arena = np.frombuffer(self.arena_head + self.packed.cpu().numpy().tobytes(), dtype=np.uint8)
        headers = self.d_headers.cpu().numpy().view(batch.HEADER_DTYPE)
        results = self.d_results.cpu().numpy().view(batch.RESULT_DTYPE)
        tabs = self.d_tabs.cpu().numpy().view(batch.DTAB_DTYPE)
        ent = self.d_ent.cpu().numpy().view(batch.HEADER_DTYPE)
        foff = self.field_off.cpu().numpy().view(np.uint32)
        self.h_results, self.h_tabs, self.h_headers, self.h_ent = results, tabs, headers, ent

        def resolve(recs):
            no, nl, vo, vl = (recs[k].astype(np.int64) for k in ("name_off", "name_len", "value_off", "value_len"))
            assert not len(recs) or (no + nl <= arena.size).all() and (vo + vl <= arena.size).all()
            return [(arena[a : a + x].tobytes(), arena[b : b + y].tobytes()) for a, x, b, y in zip(no, nl, vo, vl)]

        out = []
        for d, (tab, _) in enumerate(self.decoders):
            res = []
            for b in self.lists[d]:
                r = results[b]
                if d not in void:
                    assert r["first_header"] == foff[b] and r["n_headers"] <= foff[b + 1] - foff[b]
                res.append((resolve(headers[foff[b] : foff[b] + r["n_headers"]]), int(r["error"]), int(r["detail"])))
            t = tabs[d]
            assert t["ent"] == self.used_tabs[d]["ent"] and t["cap"] == self.used_tabs[d]["cap"] and t["reserved"] == 0
            if d in void:
                out.append((res, int(t["applied"]), t))
                continue
            assert t["count"] <= t["cap"]
            after = ac.Table(resolve(ent[t["ent"] : t["ent"] + t["count"]]), int(t["max_size"]), tab.max_allowed, tab.cap)
            assert after.size == t["size"], d
            out.append((res, int(t["applied"]), after))
        return out


def run(codec, decoders, ring, **kw):
    call = Call(codec, decoders, ring, **kw).scan()
    call.apply()
    return call.fetch()


def check(got, decoders, ring, tables=True):
    """against ref_apply on copies of the tables -> (results, applied, Table) per decoder as ref_apply has them"""
    tabs = ac.fresh(decoders)
    want = ac.ref_apply(tabs, ring)
    assert len(got) == len(want)
    for d, ((res, applied, after), (wres, wapplied), (tab, blocks)) in enumerate(zip(got, want, tabs)):
        assert applied == wapplied, d
        for b, (g, w) in enumerate(zip(res, wres)):
            assert g == w, (d, b, blocks[b].hex()[:80], g[1:], w[1:])
        assert len(res) == len(wres)
        if tables:
            assert after.entries == tab.entries and after.max_size == tab.max_size and after.size == tab.size, d
    return [(wres, wapplied, tab) for (wres, wapplied), (tab, _) in zip(want, tabs)]


def test_interop_stories_one_call(codec, geo):
    """all 159 stories in one call, their blocks interleaved: every header against the fixture's lists (which the
    CPU tests pin ref_apply and the oracle to), nothing deferred; the final tables against ref_apply for every
    sixth story (the model takes seconds for all of them)"""
    ring, _ = geo
    stories = [s for _, s in bc.stories()]
    decoders = [(ac.Table(), [bytes.fromhex(c["wire"]) for c in s["cases"]]) for s in stories]
    call = Call(codec, decoders, ring).scan()
    assert len(call.blocks) > 16000 and call.nf > 190000
    call.apply()
    got = call.fetch()
    for (res, applied, after), s in zip(got, stories):
        assert applied == len(s["cases"])
        for (headers, error, detail), c in zip(res, s["cases"]):
            assert (error, detail) == (0, 0)
            assert headers == [(n.encode(), v.encode()) for n, v in c["headers"]]
        assert after.size <= after.max_size
    check(got[::6], decoders[::6], ring)
    assert not (call.h_results["error"] == ac.E_DEFERRED).any()


@pytest.mark.parametrize("seed,nstories", [(7541, 40), (9, 12)])
def test_corrupted_stories(codec, geo, seed, nstories):
    ring, _ = geo
    decoders = [(ac.Table(), blocks) for blocks in bc.corrupted_stories(seed=seed, nstories=nstories)]
    want = check(run(codec, decoders, ring), decoders, ring)
    assert all(applied == len(blocks) for (_, applied, _), (_, blocks) in zip(want, decoders))
    assert sum(e != 0 for res, _, _ in want for _, e, _ in res) > (20 if nstories == 40 else 5)


def test_random_and_placed_blocks_one_decoder_each(codec, geo):
    ring, _ = geo
    decoders = [(ac.Table(), [w]) for w in bc.random_blocks() + [b for _, b, _ in bc.placed()]]
    assert len(decoders) == 3331
    got = run(codec, decoders, ring)
    want = check(got, decoders, ring)
    deferred = [d for d, (_, applied, _) in enumerate(got) if applied == 0]
    assert deferred == [d for d, (_, applied, _) in enumerate(want) if applied == 0]
    assert len(deferred) == (5 if ring == 128 else 3)
    assert len({e for res, _, _ in want for _, e, _ in res}) >= 7


def test_every_truncation_of_rfc_blocks(codec, geo):
    ring, _ = geo
    decoders = [(ac.primed_table(size, before), [w]) for size, before, w in ac.rfc_truncations()]
    assert sum(len(t.entries) > 0 for t, _ in decoders) > 100
    want = check(run(codec, decoders, ring), decoders, ring)
    assert sum(e != 0 for res, _, _ in want for _, e, _ in res) > 50


@pytest.mark.parametrize("calls", [2, 3])
def test_calls_carry_the_tables(codec, geo, calls):
    """the tables that come back in tabs / tab_ent go into the next call"""
    ring, _ = geo
    stories = [[bytes.fromhex(c["wire"]) for c in s["cases"]] for _, s in list(bc.stories())[:: 159 // 12][:12]]
    stories += bc.corrupted_stories(seed=9, nstories=6)
    tabs = [ac.Table() for _ in stories]
    model = [ac.Table() for _ in stories]
    for c in range(calls):
        part = [blocks[len(blocks) * c // calls : len(blocks) * (c + 1) // calls] for blocks in stories]
        got = run(codec, list(zip(tabs, part)), ring)
        check(got, list(zip(model, part)), ring)
        ac.ref_apply(list(zip(model, part)), ring)
        tabs = [after for _, _, after in got]
        assert [t.entries for t in tabs] == [t.entries for t in model]
    assert sum(len(t.entries) for t in tabs) > 100


def test_placed_cases(codec, geo):
    ring, chunk = geo
    cases = ac.placed(ring, chunk)
    decoders = [(tab, blocks) for _, tab, blocks, _ in cases]
    for order in ("interleaved", "by decoder"):
        got = run(codec, decoders, ring, order=order)
        check(got, decoders, ring)
        for (name, _, _, expect), (res, applied, after) in zip(cases, got):
            ac.check_expect(name, after, res, applied, expect)


def test_two_decoders_interleaved_and_a_void_block_from_the_scan(codec, geo):
    """decoder 0's and decoder 1's blocks alternate in the call's list; block 2's offsets decrease, so the scan
    leaves it no fields (and sets the sticky flag, read here before the apply)"""
    ring, _ = geo
    a = [ac.lit_incr(b"a%d" % k, b"x") + ac.indexed(62) for k in range(5)]
    b = [ac.lit_incr(b"b%d" % k, b"y") + ac.indexed(62 + k) for k in range(5)]
    decoders = [(ac.Table(), a), (ac.Table([ac.entry(7)]), b)]
    call = Call(codec, decoders, ring)
    assert call.lists == [[0, 2, 4, 6, 8], [1, 3, 5, 7, 9]]
    call.block_off[3] = call.block_off[2] - 1  # block 2 = [off, off - 1): void; block 3 starts one octet early
    call.scan(void_blocks=True)
    call.apply()
    got = call.fetch()
    assert got[0][0][1] == ([], 0, 0)  # the void block: no fields, no headers, no error
    model = [(ac.Table(), a[:1] + [b""] + a[2:]), (ac.Table([ac.entry(7)]), b[:1] + [b[0][-1:] + a[1] + b[1]] + b[2:])]
    check(got, model, ring)


def small_call(codec, ring):
    """three decoders, two blocks each, with carried-in entries; and what ref_apply gives for them"""
    decoders = [(ac.Table([ac.entry(k), ac.entry(k + 10)]), [ac.lit_incr(62, b"v%d" % k) + ac.indexed(63), ac.indexed(64) + ac.indexed(2)])
                for k in range(3)]
    return Call(codec, decoders, ring, order="by decoder").scan(), decoders


def expect_void(call, decoders, ring, void, unlisted=()):
    """the decoders in `void` are void: their listed blocks deferred (those in `unlisted` left zero), applied 0,
    their hpk_dtab records and their entries as they came; the other decoders as ref_apply has them"""
    got = call.fetch(void=void)
    for d in void:
        res, applied, t = got[d]
        for b, r in zip(call.lists[d], res):
            assert r == (([], 0, 0) if b in unlisted else ([], ac.E_DEFERRED, 0)), (d, b, r)
        assert applied == 0
        assert all(t[k] == call.used_tabs[d][k] for k in ("count", "size", "max_size", "max_allowed")), d
        e0, cap = call.tabs[d]["ent"], call.tabs[d]["cap"]  # (where its entries really lie)
        assert (call.h_ent[e0 : e0 + cap] == call.tab_ent[e0 : e0 + cap]).all(), d
    others = [d for d in range(len(decoders)) if d not in void]
    check([got[d] for d in others], [decoders[d] for d in others], ring)


def test_bad_inputs_void_one_decoder(codec, geo):
    from loona_amd import _lib

    ring, _ = geo
    call, decoders = small_call(codec, ring)
    assert call.lists == [[0, 1], [2, 3], [4, 5]]
    call.apply()
    check(call.fetch(), decoders, ring)  # the call as it stands is good
    nent = len(call.tab_ent)

    def bent_tabs(d, **fields):
        t = call.tabs.copy()
        for k, v in fields.items():
            t[d][k] = v
        return t

    foff = call.field_off.cpu().numpy().view(np.uint32).copy()
    dec_foff = foff.copy()
    dec_foff[3] = foff[4] + 1  # block 3, decoder 1's second, decreases (and its first grows): both are decoder 1's
    past_end = call.dec_blk_off.copy()
    past_end[2] = past_end[3] + 1  # decoder 1's list passes dec_blk_off[ndecs]; decoder 2's then decreases
    cases = [  # (what is bent, the void decoders, their blocks that are left zero)
        ("ent + cap passes tab_ent_cap", dict(tabs=bent_tabs(1, ent=nent - ring + 1)), (1,), ()),
        ("count above cap", dict(tabs=bent_tabs(1, cap=1)), (1,), ()),
        ("a listed block index >= nblocks", dict(dec_blk=np.where(np.arange(6) == 3, 6, call.dec_blk)), (1,), (3,)),
        ("a listed block's field_off decreases", dict(field_off=i32(dec_foff)), (1,), ()),
        ("a list passes the lists' end, the next one decreases", dict(dec_blk_off=past_end), (1, 2), (2, 3, 4, 5)),
        ("a field's str + nstr passes nstrs", dict(nstrs=call.ns - 1), (2,), ()),  # the last string is decoder 2's
        ("a listed block's field_off passes headers_cap", dict(headers_cap=call.nf - 1), (2,), ()),  # the last block too
    ]
    for name, bent, void, unlisted in cases:
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            call.apply(**bent)
        expect_void(call, decoders, ring, void, unlisted)
        call.apply(sync=False, **bent)  # the sticky flag, after an asynchronous call
        assert _lib.lib().hpk_ctx_check(codec._h) == _lib.HPK_E_INVAL, name
        assert _lib.lib().hpk_ctx_check(codec._h) == _lib.HPK_E_OK
        expect_void(call, decoders, ring, void, unlisted)


def test_headers_cap_below_the_field_total(codec, geo):
    """a block no decoder lists lies past headers_cap: HPK_E_NOSPACE from the synchronous call, the listed blocks
    complete, nothing written at or past the capacity (the guards fetch() checks)"""
    ring, _ = geo
    decoders = [(ac.Table(), [ac.long_block(70), ac.indexed(62)]), (ac.Table(), [ac.indexed(2) * 3])]
    call = Call(codec, decoders, ring, order="by decoder", unlisted=[ac.indexed(3) * 5]).scan()
    assert call.nf == 70 + 1 + 3 + 5
    with pytest.raises(RuntimeError, match=r"\(-2\)"):
        call.apply(headers_cap=call.nf - 5)
    check(call.fetch(), decoders, ring)
    assert tuple(call.h_results[3]) == (0, 0, 0, 0)  # a block in no list: zero
    call.apply(headers_cap=call.nf - 5, sync=False)  # asynchronous: the caller compares
    codec.check()
    check(call.fetch(), decoders, ring)


def test_async_then_check_and_argument_checks(codec, geo):
    from loona_amd import _lib

    ring, _ = geo
    call, decoders = small_call(codec, ring)
    call.apply(sync=False)
    assert _lib.lib().hpk_ctx_check(codec._h) == _lib.HPK_E_OK
    check(call.fetch(), decoders, ring)
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dbo, db = i32(call.dec_blk_off), i32(call.dec_blk)  # (kept alive: only their addresses go into the calls below)
    args = lambda **kw: [kw.get("ctx", codec._h), p(kw.get("fields", call.fields)), p(call.field_off), len(call.blocks),  # noqa: E731
                         p(call.out_off), p(call.out_len), p(call.status), call.ns, call.str_base,
                         kw.get("static_base", call.static_base), p(dbo), p(db), len(decoders),
                         p(call.d_tabs), p(kw.get("ent", call.d_ent)), len(call.tab_ent), p(kw.get("headers", call.d_headers)), call.nf,
                         p(call.d_results), kw.get("flags", _lib.HPK_PTR_DEVICE)]
    assert L.hpk_apply_blocks(*args(ctx=None)) == _lib.HPK_E_INVAL
    assert L.hpk_apply_blocks(*args(flags=_lib.HPK_PTR_HOST)) == _lib.HPK_E_INVAL
    assert L.hpk_apply_blocks(*args(static_base=2**32 - 600)) == _lib.HPK_E_INVAL  # the static text would pass 2^32
    for which in ("fields", "ent", "headers"):  # each must be 16-byte aligned
        whole = torch.zeros(16 * 64 + 8, dtype=torch.uint8, device="cuda")
        assert L.hpk_apply_blocks(*args(**{which: whole[8:]})) == _lib.HPK_E_INVAL, which
    assert L.hpk_test_blkapply_geometry(None, None, None) == _lib.HPK_E_INVAL
    check(call.fetch(), decoders, ring)  # (a refused call touches nothing)
    # no decoders, and no blocks: nothing but results zeroed
    g, results = guarded(16 * len(call.blocks))
    a = args()
    a[12], a[18] = 0, p(results)
    assert L.hpk_apply_blocks(*a) == _lib.HPK_E_OK
    assert not results.cpu().numpy().any() and guards_intact(g)
    a = args()
    a[3] = 0
    assert L.hpk_apply_blocks(*a) == _lib.HPK_E_OK
    check(call.fetch(), decoders, ring)  # (that call touched nothing)


def test_static_table_export():
    from loona_amd import batch

    text, ent = batch.static_table()
    got = [(text[e["name_off"] : e["name_off"] + e["name_len"]], text[e["value_off"] : e["value_off"] + e["value_len"]]) for e in ent]
    assert got == ac.static_table() and len(text) == sum(len(n) + len(v) for n, v in got)
