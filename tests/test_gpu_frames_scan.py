"""The frame scan and the fragment gather on the GPU (hpk_scan_frames, hpk_frame_blocks), record for record: no
tolerance. The expected result is frames_cases.expected_batch(): ref_scan_frames connection by connection, which
test_frames_cases.py pins to the hand-written expectations and to h2_cases._frames; never the code under test.

One checker serves every case: the block records and the fragment windows go into views of canary-filled buffers with
guards behind them, the three offset arrays are prefilled with values the call never writes; afterwards the arrays
and the states are the expected ones, the records and windows below min(total, capacity) are the expected ones, and
the canary is intact at and past that point."""

import ctypes

import numpy as np
import pytest

import frames_cases as fc
import h2_cases as hc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CANARY = 0xA5
CANARY32 = np.int32(-0x5A5A5A5B)  # 0xA5A5A5A5
GUARD = 1024
PRE_OFF = -3
BAD_OFFSETS = 5


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU)")
    from loona_amd import HuffmanCodec

    c = HuffmanCodec(0, stream=torch.cuda.current_stream())
    yield c
    c.close()


@pytest.fixture(scope="module")
def wg():
    from loona_amd import _lib

    w = ctypes.c_uint32(0)
    assert _lib.lib().hpk_test_frmscan_geometry(ctypes.byref(w)) == _lib.HPK_E_OK
    assert w.value >= 64
    return w.value


@pytest.fixture(scope="module")
def placed_items():
    return [(c.state, c.data, c.carry) for c in fc.placed()]


@pytest.fixture(scope="module")
def interop():
    """the interop connections whole, and the batch expected of them"""
    wires, wants = hc.interop_connections(4)
    return wires, wants, fc.expected_batch([(fc.State(), w, b"") for w in wires])


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(codec, x, shift=0, caps=(None, None, None), sync=True, raises=None, cap=None):
    """scan_frames on batch x with the blob `shift` bytes off a 256-byte boundary -> the outputs as numpy arrays, the
    lists whole (canaries and guards included)"""
    n = len(x.off) - 1
    size = x.blob.size if cap is None else cap
    most_b = (int(x.off[n]) - int(x.off[0])) // 9 if n else 0
    bcap = most_b if caps[0] is None else caps[0]
    fcap = most_b + n if caps[1] is None else caps[1]
    ocap = most_b + n if caps[2] is None else caps[2]
    src = np.zeros(shift + x.blob.size + 1, np.uint8)
    src[shift : shift + x.blob.size] = x.blob
    dblob = to_dev(src)[shift : shift + size]
    doff = to_dev(x.off.view(np.int32))
    dconns = to_dev(x.conns.view(np.uint8).reshape(-1)) if n else torch.zeros(0, dtype=torch.uint8, device="cuda")
    bbig = torch.full((16 * bcap + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    mk = lambda m: torch.full((m + GUARD,), int(CANARY32), dtype=torch.int32, device="cuda")  # noqa: E731
    fo, fl, oo, ol = mk(fcap), mk(fcap), mk(ocap), mk(ocap)
    cb, cf, co = (torch.full((n + 1,), PRE_OFF, dtype=torch.int32, device="cuda") for _ in range(3))
    kw = dict(blocks=bbig[: 16 * bcap], conn_blk_off=cb, frag_off=fo[:fcap], frag_len=fl[:fcap], conn_frag_off=cf, open_off=oo[:ocap],
              open_len=ol[:ocap], conn_open_off=co)
    if raises is None:
        codec.scan_frames(dblob, doff, dconns, sync=sync, **kw)
        if not sync:
            codec.check()
    else:
        with pytest.raises(RuntimeError, match=raises):
            codec.scan_frames(dblob, doff, dconns, sync=True, **kw)
    torch.cuda.synchronize()
    u = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    return dict(conns=dconns.cpu().numpy().view(fc.FCONN_DTYPE), blocks=bbig.cpu().numpy(), fo=fo.cpu().numpy(), fl=fl.cpu().numpy(),
                oo=oo.cpu().numpy(), ol=ol.cpu().numpy(), cb=u(cb), cf=u(cf), co=u(co), caps=(bcap, fcap, ocap))


def compare(what, x, g, void=()):
    bcap, fcap, ocap = g["caps"]
    assert np.array_equal(g["cb"], x.conn_blk_off), f"{what}: conn_blk_off"
    assert np.array_equal(g["cf"], x.conn_frag_off), f"{what}: conn_frag_off"
    assert np.array_equal(g["co"], x.conn_open_off), f"{what}: conn_open_off"
    want = x.conns_out.copy()
    for k in void:  # untouched apart from status
        want[k] = x.conns[k]
        want[k]["status"] = BAD_OFFSETS
    if not np.array_equal(g["conns"], want):
        k = int(np.nonzero(g["conns"] != want)[0][0])
        raise AssertionError(f"{what}: connection {k}: {g['conns'][k]} for {want[k]}")
    nb, nf, no = min(len(x.blocks), bcap), min(len(x.frag_off), fcap), min(len(x.open_off), ocap)
    gb = g["blocks"][: 16 * nb].view(fc.FBLOCK_DTYPE)
    if not np.array_equal(gb, x.blocks[:nb]):
        i = int(np.nonzero(gb != x.blocks[:nb])[0][0])
        raise AssertionError(f"{what}: block {i}: {gb[i]} for {x.blocks[i]}")
    assert np.array_equal(g["fo"][:nf].view(np.uint32), x.frag_off[:nf]), f"{what}: frag_off"
    assert np.array_equal(g["fl"][:nf].view(np.uint32), x.frag_len[:nf]), f"{what}: frag_len"
    assert np.array_equal(g["oo"][:no].view(np.uint32), x.open_off[:no]), f"{what}: open_off"
    assert np.array_equal(g["ol"][:no].view(np.uint32), x.open_len[:no]), f"{what}: open_len"
    assert (g["blocks"][16 * nb :] == CANARY).all(), f"{what}: records at or past min(total, blocks_cap) were written"
    assert (g["fo"][nf:] == CANARY32).all() and (g["fl"][nf:] == CANARY32).all(), f"{what}: closed windows past the capacity"
    assert (g["oo"][no:] == CANARY32).all() and (g["ol"][no:] == CANARY32).all(), f"{what}: open windows past the capacity"


def compare_host(what, x, got):
    conns, blocks, cb, fo, fl, cf, oo, ol, co = got
    assert np.array_equal(cb, x.conn_blk_off) and np.array_equal(cf, x.conn_frag_off) and np.array_equal(co, x.conn_open_off), what
    assert np.array_equal(conns, x.conns_out), f"{what}: states"
    assert np.array_equal(blocks, x.blocks), f"{what}: blocks"
    assert np.array_equal(fo, x.frag_off) and np.array_equal(fl, x.frag_len), f"{what}: closed windows"
    assert np.array_equal(oo, x.open_off) and np.array_equal(ol, x.open_len), f"{what}: open windows"


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_placed_cases_at_four_alignments(codec, placed_items, shift):
    x = fc.expected_batch(placed_items, base=shift)
    assert len(x.blocks) > 20 and len(x.open_off) > 10 and set(x.conns_out["error"]) == set(range(9))
    compare(f"placed, device, shift {shift}", x, run(codec, x, shift=shift))
    compare(f"placed, device, data from {shift}", x, run(codec, x, shift=(4 - shift) % 4))
    compare_host(f"placed, host, base {shift}", x, codec.scan_frames_host(x.blob, x.off, x.conns))


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("n", ["0", "1", "wg-1", "wg", "wg+1"])
def test_connection_counts_at_the_workgroup(codec, wg, interop, placed_items, n, where):
    """connection counts on each side of a workgroup, the longest connection in the first and in the last lane"""
    n = {"wg-1": wg - 1, "wg": wg, "wg+1": wg + 1}.get(n) or int(n)
    wires = interop[0]
    long = max(wires, key=len)
    small = [placed_items[k % len(placed_items)] for k in range(max(n - 1, 0))]
    items = ([(fc.State(), long, b"")] + small if where == "first" else small + [(fc.State(), long, b"")])[:n] if n else []
    if n and where == "last":
        items[-1] = (fc.State(), long, b"")
    x = fc.expected_batch(items)
    compare(f"{n} connections", x, run(codec, x))
    compare(f"{n} connections, async", x, run(codec, x, sync=False))
    compare_host(f"{n} connections, host", x, codec.scan_frames_host(x.blob, x.off, x.conns))
    if n == 0:
        assert list(x.conn_blk_off) == [0] and list(x.conn_frag_off) == [0] and list(x.conn_open_off) == [0]


def test_interop_connections_one_call(codec, interop):
    wires, _, x = interop
    assert len(x.blocks) > 10000
    compare("interop", x, run(codec, x))
    compare_host("interop, host", x, codec.scan_frames_host(x.blob, x.off, x.conns))


@pytest.mark.parametrize("which", [0, 1, 2])
def test_each_capacity_one_below_its_total(codec, placed_items, interop, which):
    """canaries round every output, HPK_E_NOSPACE from the synchronous calls, the arrays and the states complete"""
    x = fc.expected_batch(placed_items + [(fc.State(), w, b"") for w in interop[0][:40]])
    totals = (len(x.blocks), len(x.frag_off), len(x.open_off))
    for cap in (totals[which] - 1, 0):
        caps = [None, None, None]
        caps[which] = cap
        compare(f"capacity {which} = {cap}", x, run(codec, x, caps=caps, raises="-2"))
        compare(f"capacity {which} = {cap}, async", x, run(codec, x, caps=caps, sync=False))  # (an async call cannot say NOSPACE)
        with pytest.raises(RuntimeError, match="-2"):
            codec.scan_frames_host(x.blob, x.off, x.conns, *caps)
    caps = [None, None, None]
    caps[which] = totals[which]
    compare(f"capacity {which} exact", x, run(codec, x, caps=caps))
    compare_host(f"capacity {which} exact, host", x, codec.scan_frames_host(x.blob, x.off, x.conns, *caps))


def test_host_capacity_writes_only_below_it(codec, placed_items):
    """host pointers: exactly the written parts come back (numpy canaries behind the capacities)"""
    from loona_amd import _lib

    x = fc.expected_batch(placed_items)
    n = len(x.off) - 1
    bcap, fcap, ocap = len(x.blocks) - 2, len(x.frag_off) - 3, len(x.open_off) - 1
    b = np.full(16 * len(x.blocks) + 64, CANARY, np.uint8)
    fo = np.full(len(x.frag_off) + 16, 0xA5A5A5A5, np.uint32)
    fl, oo, ol = fo.copy(), fo.copy(), fo.copy()
    cb, cf, co = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32)
    conns = x.conns.copy()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    rc = _lib.lib().hpk_scan_frames(codec._h, p(x.blob), x.blob.size, p(x.off), n, p(conns), p(b), bcap, p(cb), p(fo), p(fl), fcap, p(cf),
                                    p(oo), p(ol), ocap, p(co), _lib.HPK_PTR_HOST)
    assert rc == _lib.HPK_E_NOSPACE
    assert np.array_equal(cb, x.conn_blk_off) and np.array_equal(cf, x.conn_frag_off) and np.array_equal(co, x.conn_open_off)
    assert np.array_equal(conns, x.conns_out)
    assert np.array_equal(b[: 16 * bcap].view(fc.FBLOCK_DTYPE), x.blocks[:bcap]) and (b[16 * bcap :] == CANARY).all()
    assert np.array_equal(fo[:fcap], x.frag_off[:fcap]) and (fo[fcap:] == 0xA5A5A5A5).all()
    assert np.array_equal(fl[:fcap], x.frag_len[:fcap]) and (fl[fcap:] == 0xA5A5A5A5).all()
    assert np.array_equal(oo[:ocap], x.open_off[:ocap]) and (oo[ocap:] == 0xA5A5A5A5).all()
    assert np.array_equal(ol[:ocap], x.open_len[:ocap]) and (ol[ocap:] == 0xA5A5A5A5).all()


@pytest.mark.parametrize("kind", ["decreasing", "past cap", "carry past cap"])
def test_void_connections(codec, placed_items, kind):
    """a connection whose offsets decrease or pass cap, or whose carry window passes cap while it is pending, is void
    (status HPK_BAD_OFFSETS, nothing else of it touched, no records, the sticky flag); its neighbours are scanned as
    they lie; the synchronous call returns HPK_E_INVAL"""
    from loona_amd import _lib

    items = list(placed_items[:48])
    pend = next(k for k, it in enumerate(items) if it[0].pending and it[2])
    x = fc.expected_batch(items)
    off = x.off.astype(np.int64)
    conns = x.conns.copy()
    cap = None
    if kind == "decreasing":
        k = 20  # connection 20 ends before it starts; 21 starts earlier, inside 20's bytes, and is read as it lies
        off[k + 1] = off[k] - 2
        void = [k]
    elif kind == "past cap":
        # the capacity ends one byte before the last connection's end; the carries lie behind it, so no pending
        # connection may follow
        items = [it for it in items if not it[0].pending]
        x = fc.expected_batch(items)
        off, conns = x.off.astype(np.int64), x.conns.copy()
        cap = int(off[-1]) - 1
        void = [len(items) - 1]
        assert len(items[-1][1]) > 0
    else:
        conns[pend]["carry_len"] = x.blob.size - int(conns[pend]["carry_off"]) + 1
        void = [pend]
    # what the scan must give: every connection as it lies now, the void ones nothing
    want_items = []
    for k, (st, _, carry) in enumerate(items):
        lo, hi = int(off[k]), int(off[k + 1])
        want_items.append((st, x.blob[lo:hi].tobytes() if k not in void else b"", carry))
    n = len(items)
    # the async call, then the sticky flag through check()
    dblob = to_dev(x.blob)[: x.blob.size if cap is None else cap]
    doff, dconns = to_dev(off.astype(np.uint32).view(np.int32)), to_dev(conns.view(np.uint8).reshape(-1))
    out = codec.scan_frames(dblob, doff, dconns, sync=False)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="HPK_BAD_OFFSETS"):
        codec.check()
    codec.check()  # (read and cleared)
    got_conns = dconns.cpu().numpy().view(fc.FCONN_DTYPE)
    with pytest.raises(RuntimeError, match="HPK_BAD_OFFSETS"):  # a synchronous call says so itself
        codec.scan_frames(dblob, doff, to_dev(conns.view(np.uint8).reshape(-1)), sync=True)
    blocks, cb, fo, fl, cf, oo, ol, co = out
    u = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    cb, cf, co, fo, fl, oo, ol = u(cb), u(cf), u(co), u(fo), u(fl), u(oo), u(ol)
    gb = blocks.cpu().numpy().view(fc.FBLOCK_DTYPE)
    for k in range(n):
        st, data, carry = want_items[k]
        if k in void:
            assert cb[k + 1] == cb[k] and cf[k + 1] == cf[k] and co[k + 1] == co[k], k
            want = conns[k].copy()
            want["status"] = BAD_OFFSETS
            assert got_conns[k] == want, (k, got_conns[k])
            continue
        s = fc.ref_scan_frames(st, data, carry, int(off[k]), int(conns[k]["carry_off"]))
        assert [(int(b["conn"]), int(b["stream_id"]), int(b["frag"]) - int(cf[k]), int(b["nfrag"])) for b in gb[cb[k] : cb[k + 1]]] == \
            [(k, sid, f, m) for sid, f, m in s.blocks], k
        assert list(zip(fo[cf[k] : cf[k + 1]].tolist(), fl[cf[k] : cf[k + 1]].tolist())) == s.closed, k
        assert list(zip(oo[co[k] : co[k + 1]].tolist(), ol[co[k] : co[k + 1]].tolist())) == s.open, k
        assert (got_conns[k]["error"], got_conns[k]["pending"], got_conns[k]["pend_stream"], got_conns[k]["consumed"], got_conns[k]["status"]) == \
            (s.state.error, s.state.pending, s.state.pend_stream, s.consumed, 0), k
    # the host form checks the connections before anything is copied
    before = conns.copy()
    with pytest.raises(RuntimeError, match="-1"):
        codec.scan_frames_host(x.blob[: (x.blob.size if cap is None else cap)], off.astype(np.uint32), conns)
    assert np.array_equal(conns, before)
    # cap above HPK_MAX_OFFSET
    z = torch.zeros(64, dtype=torch.int32, device="cuda")
    q = ctypes.c_void_p(z.data_ptr())
    rc = _lib.lib().hpk_scan_frames(codec._h, q, _lib.HPK_MAX_OFFSET + 1, q, 0, None, None, 0, q, None, None, 0, q, None, None, 0, q,
                                    _lib.HPK_PTR_DEVICE)
    assert rc == _lib.HPK_E_INVAL


def test_misaligned_records_are_refused(codec, placed_items):
    x = fc.expected_batch(placed_items[:8])
    n = 8
    dblob, doff = to_dev(x.blob), to_dev(x.off.view(np.int32))
    raw = torch.zeros(32 * n + 16, dtype=torch.uint8, device="cuda")
    blocks = torch.zeros(16 * 64 + 16, dtype=torch.uint8, device="cuda")
    good = raw[: 32 * n]
    good.copy_(to_dev(x.conns.view(np.uint8).reshape(-1)))
    for conns, blk in ((raw[4 : 4 + 32 * n], blocks[: 16 * 64]), (good, blocks[8 : 8 + 16 * 64])):
        for sync in (False, True):
            with pytest.raises(RuntimeError, match="16-byte aligned"):
                codec.scan_frames(dblob, doff, conns, blocks=blk, sync=sync)
    codec.check()
    # int64 offsets, a view and a host array are refused before the library sees them
    with pytest.raises(TypeError):
        codec.scan_frames(dblob, doff.to(torch.int64), good)
    with pytest.raises(ValueError):
        codec.scan_frames(dblob, to_dev(np.repeat(x.off, 2).view(np.int32))[::2], good)
    with pytest.raises(ValueError):
        codec.scan_frames(dblob, doff, x.conns.view(np.uint8).reshape(-1))
    with pytest.raises(ValueError):
        codec.scan_frames(dblob.cpu(), doff, good)


def gather(codec, x, out_cap=None, sync=True, blocks=None, raises=None):
    dblob = to_dev(x.blob)
    nf = len(x.frag_off)
    total = int(np.sum(x.frag_len.astype(np.int64)))
    cap = total if out_cap is None else out_cap
    big = torch.full((cap + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    blk = x.blocks if blocks is None else blocks
    dblk = to_dev(blk.view(np.uint8).reshape(-1)) if len(blk) else torch.zeros(0, dtype=torch.uint8, device="cuda")
    boff = torch.full((len(blk) + 1,), PRE_OFF, dtype=torch.int32, device="cuda")
    fo = to_dev(x.frag_off.view(np.int32)) if nf else torch.zeros(0, dtype=torch.int32, device="cuda")
    fl = to_dev(x.frag_len.view(np.int32)) if nf else torch.zeros(0, dtype=torch.int32, device="cuda")
    if raises is None:
        codec.frame_blocks(dblob, fo, fl, dblk, out_blob=big[:cap], block_off=boff, sync=sync)
        if not sync:
            codec.check()
    else:
        with pytest.raises(RuntimeError, match=raises):
            codec.frame_blocks(dblob, fo, fl, dblk, out_blob=big[:cap], block_off=boff, sync=True)
        codec.check()
    torch.cuda.synchronize()
    return big.cpu().numpy(), boff.cpu().numpy().view(np.uint32), cap, total


def test_frame_blocks_concatenates_the_fragments(codec, placed_items, interop):
    x = fc.expected_batch(placed_items + [(fc.State(), w, b"") for w in interop[0][:60]], base=1)
    want = b"".join(x.block_bytes)
    want_off = np.concatenate([[0], np.cumsum([len(b) for b in x.block_bytes])]).astype(np.uint32)
    for sync in (True, False):
        out, boff, cap, total = gather(codec, x, sync=sync)
        assert total == len(want) and np.array_equal(boff, want_off)
        assert out[:cap].tobytes() == want and (out[cap:] == CANARY).all()
    # one byte short: NOSPACE, block_off complete, nothing at or past the capacity
    out, boff, cap, total = gather(codec, x, out_cap=len(want) - 1, raises="-2")
    assert np.array_equal(boff, want_off) and out[:cap].tobytes() == want[:-1] and (out[cap:] == CANARY).all()
    # no fragments and no blocks
    e = fc.expected_batch([])
    out, boff, _, _ = gather(codec, e)
    assert list(boff) == [0] and (out == CANARY).all()


def test_frame_blocks_with_a_block_list_that_does_not_tile(codec, placed_items):
    """a record whose frag passes nfrags is read as nfrags, one below its predecessor's as its predecessor's; the
    sticky flag either way; the packed bytes do not depend on the records"""
    x = fc.expected_batch(placed_items)
    nf = len(x.frag_off)
    doff = np.concatenate([[0], np.cumsum(x.frag_len.astype(np.int64))]).astype(np.uint32)
    blk = x.blocks[:6].copy()
    blk["frag"] = [0, 5, 3, nf + 7, 2, nf]
    eff = [0, 5, 5, nf, nf, nf]  # (4: below its predecessor's, itself clamped to nf)
    out, boff, cap, total = gather(codec, x, blocks=blk, raises="HPK_BAD_OFFSETS")
    assert list(boff) == [int(doff[f]) for f in eff] + [int(doff[nf])]
    assert out[:cap].tobytes() == b"".join(x.blob[int(o) : int(o) + int(m)].tobytes() for o, m in zip(x.frag_off, x.frag_len))
    # a list that skips fragments but keeps the order is not an error
    blk["frag"] = [0, 2, 2, 9, 11, nf]
    out, boff, cap, total = gather(codec, x, blocks=blk)
    assert list(boff) == [int(doff[f]) for f in blk["frag"]] + [int(doff[nf])]
    # a fragment window past the blob counts 0 bytes and sets the flag (hpk_pack_batch's rule)
    y = x._replace(frag_len=x.frag_len.copy())
    y.frag_len[3] = x.blob.size
    gather(codec, y, out_cap=int(np.sum(x.frag_len.astype(np.int64))), raises="HPK_BAD_OFFSETS")


def test_the_chain_on_device_pointers(codec, interop):
    """scan_frames -> frame_blocks -> scan_blocks -> decode_strings -> apply_blocks on the interop connections in one
    call each, nothing but totals read back in between: the fixtures' header lists"""
    from loona_amd import batch

    wires, wants, x = interop
    n = len(wires)
    dblob, doff = to_dev(x.blob), to_dev(x.off.view(np.int32))
    dconns = to_dev(x.conns.view(np.uint8).reshape(-1))
    blocks, cb, fo, fl, cf, oo, ol, co = codec.scan_frames(dblob, doff, dconns, sync=True)
    nb, nf = int(cb[n].item()), int(cf[n].item())
    assert nb == len(x.blocks) and int(co[n].item()) == 0
    blk, boff = codec.frame_blocks(dblob, fo[:nf], fl[:nf], blocks, nblocks=nb, sync=True)
    fields, foff, so, se, soff, st = codec.scan_blocks(blk, boff, sync=True)
    ns, nfields = int(soff[nb].item()), int(foff[nb].item())
    fields = fields[: 16 * nfields]
    out, so_off, so_len, _, sst = codec.decode_strings(blk, so[:ns], se[:ns], sync=True)
    # one decoder per connection: its blocks are conn_blk_off[c] .. conn_blk_off[c + 1], in order
    from loona_amd import _lib

    geo = [ctypes.c_uint32(0) for _ in range(3)]
    assert _lib.lib().hpk_test_blkapply_geometry(*[ctypes.byref(g) for g in geo]) == _lib.HPK_E_OK
    per = geo[0].value  # the entries a table may grow to: the ring's, so that nothing is deferred
    text, _ = batch.static_table()
    tabs = np.zeros(n, batch.DTAB_DTYPE)
    tabs["ent"] = np.arange(n) * per
    tabs["cap"] = per
    tabs["max_size"] = 4096
    tabs["max_allowed"] = _lib.HPK_DTAB_NO_LIMIT
    dtabs = to_dev(tabs.view(np.uint8).reshape(-1))
    tab_ent = torch.zeros(16 * per * n, dtype=torch.uint8, device="cuda")
    str_base = len(text)
    headers, results = codec.apply_blocks(fields, foff, so_off, so_len, sst, ns, str_base, 0, cb, torch.arange(nb, dtype=torch.int32, device="cuda"),
                                          dtabs, tab_ent, sync=True)
    arena = text + out.cpu().numpy().tobytes()
    res = results.cpu().numpy().view(batch.RESULT_DTYPE)[:nb]
    hdr = headers.cpu().numpy().view(batch.HEADER_DTYPE)
    assert not res["error"].any()
    got = [[] for _ in wires]
    for b in range(nb):
        hl = [(arena[h["name_off"] : h["name_off"] + h["name_len"]], arena[h["value_off"] : h["value_off"] + h["value_len"]])
              for h in hdr[res[b]["first_header"] : res[b]["first_header"] + res[b]["n_headers"]]]
        got[int(x.blocks[b]["conn"])].append((int(x.blocks[b]["stream_id"]) & 0x7FFFFFFF, bool(int(x.blocks[b]["stream_id"]) >> 31), hl))
    assert got == wants
