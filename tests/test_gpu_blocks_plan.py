"""The header-block plan on the GPU (hpk_plan_blocks through HuffmanCodec.plan_blocks), record for record: no
tolerance. The arena (the static text, the carried-in entries' bytes, the fields, the prefix area) lies on the device;
the items that come back go through pack and encode_strings as a device-resident caller would send them, and the
bytes are compared block by block with hpack_ref.Encoder. The records, the items resolved to bytes and the tables
entry by entry are compared with blocks_plan_cases.ref_plan (pinned to hpack_ref.Encoder by
tests/test_blocks_plan_cases.py; the same corpora run through the real header on the CPU in
tests/test_blkplan_emulation.py)."""

import ctypes

import numpy as np
import pytest

import blocks_apply_cases as ac
import blocks_plan_cases as pc
from hpk_util import hpack_ref

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

    v = [ctypes.c_uint32() for _ in range(4)]
    assert _lib.lib().hpk_test_blkplan_geometry(*[ctypes.byref(x) for x in v]) == _lib.HPK_E_OK
    r, c, w, g = [x.value for x in v]
    assert r >= 128 and r & (r - 1) == 0 and c == 64 and w >= 1 and g == 64
    return r, c, g


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
    """one hpk_plan_blocks call over encoders [(Table, [block], huffman)], every piece kept so that a test can bend it"""

    def __init__(self, codec, encoders, ring, order="interleaved", unlisted=()):
        from loona_amd import batch

        self.codec, self.encoders, self.ring = codec, encoders, ring
        where = [(k, e) for e, (_, blocks, _) in enumerate(encoders) for k in range(len(blocks))]
        if order == "interleaved":
            where.sort()
        self.blocks = [encoders[e][1][k] for k, e in where] + list(unlisted)
        lists = [[] for _ in encoders]
        for b, (k, e) in enumerate(where):
            lists[e].append(b)
        self.lists = lists
        self.enc_blk = np.array([b for lst in lists for b in lst], dtype=np.uint32)
        self.enc_blk_off = np.concatenate([[0], np.cumsum([len(lst) for lst in lists])]).astype(np.uint32)
        self.enc_flags = np.array([2 * (e % 2) + int(h) for e, (_, _, h) in enumerate(encoders)], dtype=np.uint8)  # bit 1 is ignored
        self.hdr_off = np.concatenate([[0], np.cumsum([len(b) for b in self.blocks])]).astype(np.uint32)
        self.nh = int(self.hdr_off[-1])
        strs = [s for blk in self.blocks for n, v in blk for s in (n, v)]
        self.field_off = np.concatenate([[0], np.cumsum([len(s) for s in strs])]).astype(np.uint32)
        # the arena: 16 bytes nobody refers to, the static text, the carried-in entries' bytes, the fields, the prefix area
        text, _ = batch.static_table()
        self.static_base = 16
        prior = b"".join(n + v for tab, _, _ in encoders for n, v in tab.entries)
        self.prior_base = self.static_base + len(text) + 5
        self.fields_base = self.prior_base + len(prior) + 3
        head = bytes(16) + text + bytes(5) + prior + bytes(3) + b"".join(strs)
        head += bytes(-len(head) % 4)
        self.prefix_base = len(head)
        self.arena0 = np.frombuffer(head + b"\xee" * (4 * self.nh) + bytes(7), dtype=np.uint8).copy()
        tabs = np.zeros(len(encoders), dtype=batch.DTAB_DTYPE)
        ents = []
        at, e0 = self.prior_base, 0
        for e, (tab, _, _) in enumerate(encoders):
            cap = max(ring, len(tab.entries)) if tab.cap is None else tab.cap
            tabs[e] = (e0, cap, len(tab.entries), tab.size, tab.max_size, 0x12345678, 0xDDDDDDDD, 0)  # max_allowed is ignored
            rec = np.zeros(cap, dtype=batch.HEADER_DTYPE)
            for i, (n, v) in enumerate(tab.entries):
                rec[i] = (at, len(n), at + len(n), len(v))
                at += len(n) + len(v)
            ents.append(rec)
            e0 += cap
        self.tabs = tabs
        self.tab_ent = np.concatenate(ents) if ents else np.zeros(0, dtype=batch.HEADER_DTYPE)

    def plan(self, sync=True, **bent):
        """-> the return of plan_blocks; the outputs are kept as device tensors with guards around them"""
        nh = self.nh
        self.g_arena, arena = guarded(len(self.arena0))
        arena.copy_(torch.from_numpy(self.arena0).cuda())
        self.g_reps, reps = guarded(16 * nh)
        self.g_off, ioff = guarded(12 * nh)
        self.g_len, ilen = guarded(12 * nh)
        self.g_pol, ipol = guarded(3 * nh)
        self.g_tabs, tabs = guarded(32 * len(self.encoders))
        self.g_ent, ent = guarded(16 * len(self.tab_ent))
        self.used_tabs = bent.get("tabs", self.tabs)
        tabs.copy_(torch.from_numpy(self.used_tabs.view(np.uint8)).cuda())
        self.used_ent = bent.get("tab_ent", self.tab_ent)
        ent.copy_(torch.from_numpy(self.used_ent.view(np.uint8)).cuda())
        self.d_arena, self.d_reps, self.d_tabs, self.d_ent = arena, reps, tabs, ent
        self.d_off, self.d_len, self.d_pol = ioff.view(torch.int32), ilen.view(torch.int32), ipol
        self.d_field_off = i32(bent.get("field_off", self.field_off))
        self.d_hdr_off = i32(bent.get("hdr_off", self.hdr_off))
        self.d_lists = (i32(bent.get("enc_blk_off", self.enc_blk_off)), i32(bent.get("enc_blk", self.enc_blk)),
                        torch.from_numpy(self.enc_flags).cuda())
        return self.codec.plan_blocks(bent.get("arena", arena), self.static_base, bent.get("fields_base", self.fields_base),
                                      self.prefix_base, self.d_field_off, self.d_hdr_off, *self.d_lists, tabs, ent, reps=reps,
                                      item_off=self.d_off, item_len=self.d_len, item_policy=ipol, sync=sync)

    def encode(self):
        """the items through pack and encode_strings on the device -> the blocks' bytes"""
        c = self.codec
        if self.nh == 0:
            return [b""] * len(self.blocks)
        blob, off = c.pack(self.d_arena, self.d_off, self.d_len, sync=True)
        out, oo, _, st = c.encode_strings(blob, off, self.d_pol, sync=True)
        assert not st[: 3 * self.nh].cpu().numpy().any()
        out, oo = out.cpu().numpy(), oo.cpu().numpy().view(np.uint32)
        at = oo[3 * self.hdr_off.astype(np.int64)]
        return [out[int(a) : int(b)].tobytes() for a, b in zip(at[:-1], at[1:])]

    def fetch(self, void=()):
        """the outputs on the host, every reference resolved against the arena -> [(results, planned, Table)] in
        ref_plan's form (a block whose headers all kept their defaults is None if its encoder planned nothing); for
        an encoder in `void` the raw hpk_dtab record instead of the Table"""
        from loona_amd import batch

        assert all(guards_intact(g) for g in (self.g_arena, self.g_reps, self.g_off, self.g_len, self.g_pol, self.g_tabs, self.g_ent))
        arena = self.d_arena.cpu().numpy()
        # the arena is unchanged outside the prefix area
        assert (arena[: self.prefix_base] == self.arena0[: self.prefix_base]).all()
        assert (arena[self.prefix_base + 4 * self.nh :] == self.arena0[self.prefix_base + 4 * self.nh :]).all()
        reps = self.d_reps.cpu().numpy().view(batch.HREP_DTYPE)
        ioff = self.d_off.cpu().numpy().view(np.uint32).astype(np.int64)
        ilen = self.d_len.cpu().numpy().view(np.uint32).astype(np.int64)
        ipol = self.d_pol.cpu().numpy()
        tabs = self.d_tabs.cpu().numpy().view(batch.DTAB_DTYPE)
        ent = self.d_ent.cpu().numpy().view(batch.HEADER_DTYPE)
        self.h_reps, self.h_tabs, self.h_ent, self.h_arena = reps, tabs, ent, arena
        assert (ioff + ilen <= arena.size).all() and not reps["reserved0"].any() and not reps["reserved1"].any()

        def header(j):
            r = reps[j]
            items = [(int(ipol[3 * j + k]), arena[ioff[3 * j + k] : ioff[3 * j + k] + ilen[3 * j + k]].tobytes()) for k in range(3)]
            prefix = bytes(r["prefix"][: r["prefix_len"]])
            if r["kind"] != pc.NONE:  # slot 0 is the prefix area's dword of this header
                assert ioff[3 * j] == self.prefix_base + 4 * j and items[0] == (pc.VERBATIM, prefix)
                assert arena[ioff[3 * j] : ioff[3 * j] + 4].tobytes() == bytes(r["prefix"])
            return int(r["kind"]), int(r["index"]), prefix, items

        def resolve(recs):
            no, nl, vo, vl = (recs[k].astype(np.int64) for k in ("name_off", "name_len", "value_off", "value_len"))
            assert not len(recs) or (no + nl <= arena.size).all() and (vo + vl <= arena.size).all()
            return [(arena[a : a + x].tobytes(), arena[b : b + y].tobytes()) for a, x, b, y in zip(no, nl, vo, vl)]

        out = []
        for e, (tab, _, _) in enumerate(self.encoders):
            t = tabs[e]
            res = [[header(j) for j in range(self.hdr_off[b], self.hdr_off[b + 1])] for b in self.lists[e]]
            if t["applied"] == 0:
                assert all(h == pc.DEFAULT for blk in res for h in blk), e
                res = [None] * len(res)
            assert t["ent"] == self.used_tabs[e]["ent"] and t["cap"] == self.used_tabs[e]["cap"] and t["reserved"] == 0
            assert t["max_allowed"] == self.used_tabs[e]["max_allowed"]
            if e in void:
                out.append((res, int(t["applied"]), t))
                continue
            assert t["count"] <= t["cap"]
            after = ac.Table(resolve(ent[t["ent"] : t["ent"] + t["count"]]), int(t["max_size"]), None, tab.cap)
            assert after.size == t["size"], e
            out.append((res, int(t["applied"]), after))
        return out


def check(got, encoders, ring):
    """against ref_plan on copies of the tables -> ref_plan's results and the tables after it"""
    tabs = pc.fresh(encoders)
    want = pc.ref_plan(tabs, ring)
    assert len(got) == len(want)
    for e, ((res, planned, after), (wres, wplanned), (tab, blocks, _)) in enumerate(zip(got, want, tabs)):
        assert planned == wplanned, e
        assert len(res) == len(wres)
        for b, (g, w) in enumerate(zip(res, wres)):
            assert g == w, (e, b, blocks[b][:3])
        assert after.entries == tab.entries and after.max_size == tab.max_size and after.size == tab.size, e
    return want, tabs


def reference_bytes(encoders, want):
    """hpack_ref.Encoder's bytes for the blocks of every encoder that planned (None for a deferred encoder's)"""
    out = []
    for (tab, blocks, huffman), (_, planned) in zip(encoders, want):
        if planned == 0:
            out.append([None] * len(blocks))
            continue
        enc = hpack_ref.Encoder(huffman=huffman)
        enc.dynamic.max_size, enc.dynamic.table, enc.dynamic.size = tab.max_size, list(tab.entries), tab.size
        out.append([enc.encode(blk) for blk in blocks])
    return out


def run(codec, encoders, ring, **kw):
    """plan, fetch and check against ref_plan; then the device's pack and encode_strings against hpack_ref.Encoder"""
    call = Call(codec, encoders, ring, **kw)
    call.plan()
    got = call.fetch()
    want, tabs = check(got, encoders, ring)
    wire = call.encode()
    for e, ref in enumerate(reference_bytes(encoders, want)):
        for b, w in zip(call.lists[e], ref):
            assert wire[b] == (b"" if w is None else w), (e, b)
    return call, got, want


def test_interop_stories_one_call(codec, geo):
    """all 159 stories in one call, one encoder per story, their blocks interleaved, every other encoder Huffman-coding"""
    ring, chunk, group = geo
    encoders = pc.corpora(ring, chunk, group)["interop"]
    assert len(encoders) == 159
    call, got, want = run(codec, encoders, ring)
    assert len(call.blocks) > 16000 and call.nh > 190000
    assert all(planned == len(blocks) for (_, planned, _), (_, blocks, _) in zip(got, encoders))
    kinds = np.bincount(call.h_reps["kind"], minlength=4)
    assert kinds[pc.NONE] == 0 and kinds[1:].min() > 500


def test_random_lists(codec, geo):
    ring, chunk, group = geo
    run(codec, pc.corpora(ring, chunk, group)["random"], ring)


def test_placed_cases(codec, geo):
    ring, chunk, group = geo
    cases = pc.placed(ring, chunk, group)
    encoders = [(tab, blocks, huffman) for _, tab, blocks, huffman, _ in cases]
    for order in ("interleaved", "by encoder"):
        _, got, _ = run(codec, encoders, ring, order=order)
        for (name, _, _, _, expect), (res, planned, after) in zip(cases, got):
            pc.check_expect(name, after, res, planned, expect)


@pytest.mark.parametrize("calls", [2, 3])
def test_calls_carry_the_tables(codec, geo, calls):
    """the tables that come back in tabs / tab_ent go into the next call (their bytes laid out afresh by the caller)"""
    ring, chunk, group = geo
    stories, tabs = pc.carried(ring)  # the case the model's and the emulation's tests carry too
    model = [t.copy() for t in tabs]
    for c in range(calls):
        part = [blocks[len(blocks) * c // calls : len(blocks) * (c + 1) // calls] for blocks, _ in stories]
        _, got, _ = run(codec, [(t, p, h) for t, p, (_, h) in zip(tabs, part, stories)], ring)
        pc.ref_plan([(t, p, h) for t, p, (_, h) in zip(model, part, stories)], ring)
        tabs = [after for _, _, after in got]
        assert [t.entries for t in tabs] == [t.entries for t in model]
    assert sum(len(t.entries) for t in tabs) > 0  # (tables stay small: the strategy adds an entry only for a new name)


def small_call(codec, ring, **kw):
    """three encoders, two blocks each, with carried-in entries"""
    encoders = [(ac.Table([ac.entry(k), ac.entry(k + 10)]), [[ac.entry(k), (b"x-new%d" % k, b"v"), (b":method", b"GET")],
                                                             [(b"x-new%d" % k, b"v"), (ac.entry(k + 10)[0], b"other")]], k == 1)
                for k in range(3)]
    return Call(codec, encoders, ring, order="by encoder", **kw), encoders


def expect_void(call, encoders, ring, void):
    """the encoders in `void` are void: their headers keep the defaults, applied 0, their hpk_dtab records and their
    entries as they came; the other encoders as ref_plan has them"""
    got = call.fetch(void=void)
    for e in void:
        res, planned, t = got[e]
        assert planned == 0 and all(r is None for r in res)
        assert all(t[k] == call.used_tabs[e][k] for k in ("count", "size", "max_size")), e
        e0, cap = call.tabs[e]["ent"], call.tabs[e]["cap"]
        assert (call.h_ent[e0 : e0 + cap] == call.used_ent[e0 : e0 + cap]).all(), e
    others = [e for e in range(len(encoders)) if e not in void]
    check([got[e] for e in others], [encoders[e] for e in others], ring)


def test_bad_inputs_void_one_encoder(codec, geo):
    from loona_amd import _lib

    ring, _, _ = geo
    call, encoders = small_call(codec, ring, unlisted=[[(b"in-no", b"list")]])
    assert call.lists == [[0, 1], [2, 3], [4, 5]] and call.nh == 16
    call.plan()
    check(call.fetch(), encoders, ring)  # the call as it stands is good
    assert call.fetch()[0][0][0][0][0] == pc.INDEXED and tuple(call.h_reps[15])[:3] == (0, 0, 0)  # the unlisted block: defaults
    nent = len(call.tab_ent)

    def bent_tabs(e, **fields):
        t = call.tabs.copy()
        for k, v in fields.items():
            t[e][k] = v
        return t

    def bent_ent(i, **fields):
        t = call.tab_ent.copy()
        for k, v in fields.items():
            t[i][k] = v
        return t

    hoff = call.hdr_off.copy()
    hoff[3] = hoff[4] + 1  # block 3, encoder 1's second, decreases (and block 2 grows past it): both are encoder 1's
    past_cap = call.hdr_off.copy()
    past_cap[6] = call.nh + 1  # block 5, encoder 2's last, passes hdrs_cap (block 6 is in no list)
    past_end = call.enc_blk_off.copy()
    past_end[2] = past_end[3] + 1  # encoder 1's list passes enc_blk_off[nencs]; encoder 2's then decreases
    foff = call.field_off.copy()
    j = int(call.hdr_off[2])  # encoder 1's first header
    foff[2 * j + 1] = foff[2 * j] - 1 if foff[2 * j] else foff[2 * j + 2] + 1
    far = call.field_off.copy()
    far[30:] = 2**32 - 8  # the value of header 14, encoder 2's last, ends past the arena (header 15 is in no list)
    cases = [  # (what is bent, the void encoders)
        ("ent + cap passes tab_ent_cap", dict(tabs=bent_tabs(1, ent=nent - ring + 1)), (1,)),
        ("count above cap", dict(tabs=bent_tabs(1, cap=1)), (1,)),
        ("a listed block index >= nblocks", dict(enc_blk=np.where(np.arange(6) == 3, 7, call.enc_blk)), (1,)),
        ("a listed block's hdr_off decreases", dict(hdr_off=hoff), (1,)),
        ("a listed block's hdr_off passes hdrs_cap", dict(hdr_off=past_cap), (2,)),
        ("a list passes the lists' end, the next one decreases", dict(enc_blk_off=past_end), (1, 2)),
        ("a listed header's field_off decreases", dict(field_off=foff), (1,)),
        ("a listed header's fields_base + field_off passes arena_cap", dict(field_off=far), (2,)),
        ("a carried-in entry's name passes arena_cap", dict(tab_ent=bent_ent(ring, name_off=len(call.arena0) - 1)), (1,)),
        ("a carried-in entry's value passes arena_cap", dict(tab_ent=bent_ent(2 * ring + 1, value_len=2**32 - 1)), (2,)),
    ]
    for name, bent, void in cases:
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            call.plan(**bent)
        expect_void(call, encoders, ring, void)
        call.plan(sync=False, **bent)  # the sticky flag, after an asynchronous call
        assert _lib.lib().hpk_ctx_check(codec._h) == _lib.HPK_E_INVAL, name
        assert _lib.lib().hpk_ctx_check(codec._h) == _lib.HPK_E_OK
        expect_void(call, encoders, ring, void)


def test_async_then_check_and_argument_checks(codec, geo):
    from loona_amd import _lib

    ring, _, _ = geo
    call, encoders = small_call(codec, ring)
    call.plan(sync=False)
    assert _lib.lib().hpk_ctx_check(codec._h) == _lib.HPK_E_OK
    check(call.fetch(), encoders, ring)
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dbo, db, fl = call.d_lists
    args = lambda **kw: [kw.get("ctx", codec._h), p(kw.get("arena", call.d_arena)), kw.get("arena_cap", len(call.arena0)),  # noqa: E731
                         kw.get("static_base", call.static_base), call.fields_base, kw.get("prefix_base", call.prefix_base),
                         p(call.d_field_off), p(call.d_hdr_off), kw.get("nblocks", len(call.blocks)), call.nh, p(dbo), p(db), p(fl),
                         kw.get("nencs", len(encoders)), p(call.d_tabs), p(kw.get("ent", call.d_ent)), len(call.tab_ent),
                         p(kw.get("reps", call.d_reps)), p(call.d_off), p(call.d_len), p(call.d_pol), kw.get("flags", _lib.HPK_PTR_DEVICE)]
    before = [t.cpu().numpy().copy() for t in (call.d_arena, call.d_reps, call.d_tabs, call.d_ent, call.d_off, call.d_len, call.d_pol)]
    assert L.hpk_plan_blocks(*args(ctx=None)) == _lib.HPK_E_INVAL
    assert L.hpk_plan_blocks(*args(flags=_lib.HPK_PTR_HOST)) == _lib.HPK_E_INVAL
    assert L.hpk_plan_blocks(*args(arena_cap=_lib.HPK_MAX_OFFSET + 1)) == _lib.HPK_E_INVAL
    assert L.hpk_plan_blocks(*args(static_base=len(call.arena0) - 100)) == _lib.HPK_E_INVAL  # the static text would pass the arena
    assert L.hpk_plan_blocks(*args(prefix_base=call.prefix_base + 2)) == _lib.HPK_E_INVAL  # not a multiple of 4
    assert L.hpk_plan_blocks(*args(prefix_base=call.prefix_base + 8)) == _lib.HPK_E_INVAL  # the area passes the arena
    assert L.hpk_plan_blocks(*args(arena=call.g_arena[GUARD + 1 :])) == _lib.HPK_E_INVAL  # the area's address is not aligned
    for which in ("reps", "ent"):  # each must be 16-byte aligned
        whole = torch.zeros(16 * 64 + 8, dtype=torch.uint8, device="cuda")
        assert L.hpk_plan_blocks(*args(**{which: whole[8:]})) == _lib.HPK_E_INVAL, which
    assert L.hpk_test_blkplan_geometry(None, None, None, None) == _lib.HPK_E_INVAL
    torch.cuda.synchronize()
    after = [t.cpu().numpy() for t in (call.d_arena, call.d_reps, call.d_tabs, call.d_ent, call.d_off, call.d_len, call.d_pol)]
    assert all((a == b).all() for a, b in zip(before, after))  # a refused call touches nothing
    # no encoders, and no blocks: nothing but the defaults, the tables and the arena untouched
    for kw in (dict(nencs=0), dict(nblocks=0)):
        call.d_reps.fill_(0x77)
        call.d_len.fill_(0x77)
        assert L.hpk_plan_blocks(*args(**kw)) == _lib.HPK_E_OK
        got = call.fetch(void=(0, 1, 2))
        assert not call.h_reps.view(np.uint8).any() and (call.d_pol.cpu().numpy() == pc.VERBATIM).all()
        assert not call.d_len.cpu().numpy().any()
        assert all((a == b).all() for a, b in zip(before[2:4], (call.h_tabs.view(np.uint8), call.h_ent.view(np.uint8))))
        assert (call.h_arena == before[0]).all() and got
