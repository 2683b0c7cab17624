"""The frame write on the GPU (hpk_write_frames), octet for octet: no tolerance. The expected result is
frames_write_cases.expected_batch() / expected_from(): ref_write_frames block by block, which
test_frames_write_cases.py pins to hand-written octets and to the frame scan's model; never the code under test.

One checker serves every case: the wire goes into a view of a canary-filled buffer with guards on both sides, wire_off
and status are prefilled with values the call never writes; afterwards the arrays are the expected ones, the octets
below min(total, capacity) are the expected ones, and the canary is intact everywhere else."""

import ctypes
import random

import numpy as np
import pytest

import frames_cases as fc
import frames_write_cases as wc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CANARY = 0xA5
GUARD = 1024
PRE_OFF = -3
PRE_ST = 0x77


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

    t, w = ctypes.c_uint32(0), ctypes.c_uint32(0)
    assert _lib.lib().hpk_test_frmwrite_geometry(ctypes.byref(t), ctypes.byref(w)) == _lib.HPK_E_OK
    assert t.value >= 256 and t.value % 16 == 0 and w.value >= 64
    return t.value, w.value


@pytest.fixture(scope="module")
def placed_items():
    return [(c.block, c.stream_word, c.max_frame) for c in wc.placed()]


def rbytes(rng, n):
    return bytes(rng.randrange(256) for _ in range(n))


def word(rng):
    return rng.randrange(1, 2**31) | (wc.ES_BIT if rng.random() < 0.3 else 0)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(codec, x, src_shift=0, dst_shift=0, cap=None, sync=True, raises=None, src_cap=None, want=None):
    """write_frames on batch x, the source `src_shift` and the destination `dst_shift` octets off a 256-byte boundary,
    then every output against `want` (default: x's own expectation): (wire, wire_off, status, total)"""
    wire, wire_off, status, total = want if want is not None else (x.wire, x.wire_off, x.status, x.total)
    n = len(x.block_off) - 1
    cap = total if cap is None else cap
    size = x.blob.size if src_cap is None else src_cap
    src = np.zeros(src_shift + x.blob.size + 1, np.uint8)
    src[src_shift : src_shift + x.blob.size] = x.blob
    dblob = to_dev(src)[src_shift : src_shift + size]
    big = torch.full((GUARD + dst_shift + cap + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    out = big[GUARD + dst_shift : GUARD + dst_shift + cap]
    woff = torch.full((n + 1,), PRE_OFF, dtype=torch.int32, device="cuda")
    st = torch.full((n + 8,), PRE_ST, dtype=torch.uint8, device="cuda")
    args = (dblob, to_dev(x.block_off.view(np.int32)), to_dev(x.stream_id.view(np.int32)), to_dev(x.max_frame.view(np.int32)))
    kw = dict(out_blob=out, wire_off=woff, status=st[:n])
    if raises is None:
        codec.write_frames(*args, sync=sync, **kw)
        if not sync:
            codec.check()
    else:
        with pytest.raises(RuntimeError, match=raises):
            codec.write_frames(*args, sync=True, **kw)
    torch.cuda.synchronize()
    g = big.cpu().numpy()
    lim = min(total, cap)
    assert np.array_equal(woff.cpu().numpy().view(np.uint32), wire_off), "wire_off"
    assert np.array_equal(st.cpu().numpy()[:n], status) and (st.cpu().numpy()[n:] == PRE_ST).all(), "status"
    body = g[GUARD + dst_shift : GUARD + dst_shift + lim]
    if not np.array_equal(body, wire[:lim]):
        k = int(np.nonzero(body != wire[:lim])[0][0])
        raise AssertionError(f"wire octet {k} of {lim}: {body[k]:#x} for {wire[k]:#x} (block {int(np.searchsorted(wire_off, k, 'right')) - 1})")
    assert (g[: GUARD + dst_shift] == CANARY).all(), "octets before the blob were written"
    assert (g[GUARD + dst_shift + lim :] == CANARY).all(), "octets at or past min(total, out_cap) were written"


def run_host(codec, x, cap=None):
    out, woff, st = codec.write_frames_host(x.blob, x.block_off, x.stream_id, x.max_frame, out_cap=cap)
    assert np.array_equal(woff, x.wire_off) and np.array_equal(st, x.status)
    assert np.array_equal(out, x.wire)


@pytest.mark.parametrize("shift", [0, 1, 5, 15])
def test_placed_cases_at_shifted_blobs(codec, placed_items, shift):
    x = wc.expected_batch(placed_items, base=shift)
    assert x.wire.tobytes() == b"".join(c.wire for c in wc.placed())
    run(codec, x, src_shift=shift, dst_shift=0)
    run(codec, x, src_shift=0, dst_shift=shift)
    run(codec, x, src_shift=(16 - shift) % 16, dst_shift=shift, sync=False)  # HPK_ASYNC, then hpk_ctx_check
    run_host(codec, x)


def test_strides_around_the_chunk(codec):
    """M = 1, 6, 7, 8: frame strides 10, 15, 16 and 17 against the 16-byte chunk, L from 0 to four strides"""
    rng = random.Random(1)
    items = [(rbytes(rng, n), word(rng), m) for m in (1, 6, 7, 8) for n in range(0, 4 * (m + 9))]
    x = wc.expected_batch(items, base=2)
    run(codec, x, src_shift=3, dst_shift=11)
    run_host(codec, x)


def test_header_over_a_chunk_and_a_tile_edge(codec, geo):
    tile, _ = geo
    rng = random.Random(2)
    dst_shift = 6
    # block 1's header begins 4 octets before the first tile's end; block 2's begins 4 before a chunk's end
    first = tile - dst_shift - 4 - 9
    items = [(rbytes(rng, first), word(rng), 16384), (rbytes(rng, 40), word(rng), 16), (rbytes(rng, 3), word(rng), 5),
             (rbytes(rng, 2 * tile + 100), word(rng), 1000), (rbytes(rng, 7), word(rng), 3)]
    x = wc.expected_batch(items)
    assert int(x.wire_off[1]) + dst_shift == tile - 4
    assert (int(x.wire_off[2]) + dst_shift) % 16 in range(8, 16)
    assert (int(x.wire_off[4]) + dst_shift) // tile - (int(x.wire_off[3]) + dst_shift) // tile >= 2  # one block over three tiles
    run(codec, x, dst_shift=dst_shift)
    run(codec, x, src_shift=9, dst_shift=dst_shift)
    run_host(codec, x)


def test_runs_of_empty_and_of_void_blocks(codec, geo):
    tile, lds = geo
    rng = random.Random(3)
    empties = [(rbytes(rng, 9), word(rng), 4)] + [(b"", word(rng), 1 + k % 50) for k in range(tile // 9 + 1)] + [(rbytes(rng, 9), word(rng), 4)]
    run(codec, wc.expected_batch(empties), src_shift=1, dst_shift=13)
    # more void blocks than the window holds between two valid ones: the window restages inside one tile
    voids = [(rbytes(rng, 20), word(rng), 7)] + [(b"", word(rng), 0 if k % 2 else 0x1000000) for k in range(lds + 5)] + \
        [(rbytes(rng, 20), word(rng), 7)]
    x = wc.expected_batch(voids)
    assert np.count_nonzero(x.status) == lds + 5 and x.total < tile
    run(codec, x, raises="HPK_BAD_OFFSETS")


def scan_share():
    """the blocks one workgroup of the length scan takes: hpk_scan.h's kT * kK, read from the header"""
    import os
    import re

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "loona_amd", "csrc", "hpk_scan.h")) as f:
        m = re.search(r"constexpr uint32_t kT = (\d+), kK = (\d+), kTile = kT \* kK;", f.read())
    assert m, "hpk_scan.h no longer states its tile as kT * kK"
    return int(m.group(1)) * int(m.group(2))


@pytest.mark.parametrize("n", [0, 1, scan_share() + 1])
def test_block_counts(codec, n):
    """no block, one, and one more than a workgroup of the length scan takes"""
    rng = random.Random(n)
    items = [(rbytes(rng, k % 11), word(rng), 1 + k % 7) for k in range(n)]
    x = wc.expected_batch(items)
    run(codec, x, dst_shift=5, cap=x.total + 16)
    if n:
        run_host(codec, x)
    else:
        out, woff, st = codec.write_frames_host(x.blob, x.block_off, x.stream_id, x.max_frame)
        assert woff.tolist() == [0] and out.size == 0


def test_capacity_one_below_and_inside_a_header(codec, placed_items):
    """HPK_E_NOSPACE from the synchronous calls, the canaries intact, wire_off and status complete"""
    from loona_amd import _lib

    x = wc.expected_batch(placed_items)
    for cap in (x.total - 1, int(x.wire_off[5]) + 4, 0):
        run(codec, x, dst_shift=3, cap=cap, raises="-2")
        run(codec, x, dst_shift=3, cap=cap, sync=False)  # asynchronous: no error, the caller compares
        out = np.full(cap + 64, CANARY, np.uint8)
        woff, st = np.zeros(len(placed_items) + 1, np.uint32), np.full(len(placed_items), PRE_ST, np.uint8)
        rc = _lib.lib().hpk_write_frames(codec._h, x.blob.ctypes.data, x.blob.size, x.block_off.ctypes.data, len(placed_items),
                                         x.stream_id.ctypes.data, x.max_frame.ctypes.data, out.ctypes.data, cap, woff.ctypes.data,
                                         st.ctypes.data, _lib.HPK_PTR_HOST)
        assert rc == _lib.HPK_E_NOSPACE
        assert np.array_equal(woff, x.wire_off) and not st.any()
        assert np.array_equal(out[:cap], x.wire[:cap]) and (out[cap:] == CANARY).all()


@pytest.mark.parametrize("kind", ["decreasing", "past cap", "M = 0", "M = 0x1000000"])
def test_void_blocks_void_nothing_else(codec, placed_items, kind):
    x = wc.expected_batch(placed_items + [(b"tail block", 11, 4)])
    off, mf = x.block_off.copy(), x.max_frame.copy()
    src_cap = x.blob.size
    k = 8
    if kind == "decreasing":
        off[k + 1] = off[k] - 2  # block k ends before it starts; block k + 1 is read as it lies
    elif kind == "past cap":
        src_cap = x.blob.size - 1  # the last block passes the capacity
    elif kind == "M = 0":
        mf[k] = 0
    else:
        mf[k] = 0x1000000
    y = wc.Batch(x.blob, off, x.stream_id, mf, None, None, None, None)
    want = wc.expected_from(x.blob, src_cap, off, x.stream_id, mf)
    assert np.count_nonzero(want[2]) == 1
    run(codec, y, dst_shift=7, src_cap=src_cap, want=want, raises="HPK_BAD_OFFSETS")
    # asynchronously: the sticky flag, read and cleared by check()
    with pytest.raises(RuntimeError, match="HPK_BAD_OFFSETS"):
        run(codec, y, dst_shift=7, src_cap=src_cap, want=want, sync=False)
    codec.check()
    # host pointers: checked before anything is copied, nothing written
    from loona_amd import _lib

    out, woff, st = np.full(64, CANARY, np.uint8), np.full(len(mf) + 1, 0xDEAD, np.uint32), np.full(len(mf), PRE_ST, np.uint8)
    rc = _lib.lib().hpk_write_frames(codec._h, x.blob.ctypes.data, src_cap, off.ctypes.data, len(mf), x.stream_id.ctypes.data, mf.ctypes.data,
                                     out.ctypes.data, out.size, woff.ctypes.data, st.ctypes.data, _lib.HPK_PTR_HOST)
    assert rc == _lib.HPK_E_INVAL and (out == CANARY).all() and (woff == 0xDEAD).all() and (st == PRE_ST).all()


def test_total_past_max_offset_voids_everything(codec):
    """blocks whose wire total passes HPK_MAX_OFFSET: every wire_off 0, every block void, no octet written. The
    capacity is only a number here: nothing of the source is read when nothing is written."""
    from loona_amd import _lib

    big = 2**32 // 10 + 1
    off = to_dev(np.array([0, 5, 5 + big, 5 + big + 3], np.uint32).view(np.int32))
    sid = to_dev(np.array([1, 3, 5], np.int32))
    mf = to_dev(np.array([5, 1, 5], np.int32))
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out = torch.full((4096,), CANARY, dtype=torch.uint8, device="cuda")
    woff = torch.full((4,), PRE_OFF, dtype=torch.int32, device="cuda")
    st = torch.full((3,), PRE_ST, dtype=torch.uint8, device="cuda")
    codec._follow()
    rc = _lib.lib().hpk_write_frames(codec._h, src.data_ptr(), 5 + big + 3, off.data_ptr(), 3, sid.data_ptr(), mf.data_ptr(), out.data_ptr(), 2048,
                                     woff.data_ptr(), st.data_ptr(), _lib.HPK_PTR_DEVICE)
    assert rc == _lib.HPK_E_INVAL
    assert woff.cpu().tolist() == [0, 0, 0, 0] and st.cpu().tolist() == [wc.HPK_BAD_OFFSETS] * 3
    assert (out.cpu().numpy() == CANARY).all()
    rc = _lib.lib().hpk_write_frames(codec._h, src.data_ptr(), wc.HPK_MAX_OFFSET + 1, off.data_ptr(), 3, sid.data_ptr(), mf.data_ptr(),
                                     out.data_ptr(), 2048, woff.data_ptr(), st.data_ptr(), _lib.HPK_PTR_DEVICE)
    assert rc == _lib.HPK_E_INVAL  # cap above HPK_MAX_OFFSET


@pytest.fixture(scope="module")
def stories():
    """a few hundred interop header blocks as connections: [(blocks, header lists)] per story"""
    from hpk_util import load

    inter = load("interop.json.gz")
    out = []
    for enc in sorted(inter):
        for story in inter[enc][:8]:
            cases = [c for c in story["cases"] if c["wire"]]
            out.append(([bytes.fromhex(c["wire"]) for c in cases], [[(n.encode(), v.encode()) for n, v in c["headers"]] for c in cases]))
    assert sum(len(s[0]) for s in out) >= 300
    return out


def test_round_trip_through_the_frame_scan(codec, stories):
    """write_frames -> scan_frames -> frame_blocks gives back the blob, block_off and the stream words; for a few
    connections the chain goes on through scan_blocks -> decode_strings -> apply_blocks to the header lists"""
    from loona_amd import _lib, batch

    rng = random.Random(9)
    items, conn_of = [], []
    for c, (blocks, _) in enumerate(stories):
        m = rng.choice([16, 64, 1024, 16384])  # one frame size per connection, its scan's limit
        for i, b in enumerate(blocks):
            items.append((b, (2 * i + 1) | (wc.ES_BIT if rng.random() < 0.5 else 0), m))
            conn_of.append(c)
    x = wc.expected_batch(items)
    n, nconn = len(items), len(stories)
    dblob, dboff = to_dev(x.blob), to_dev(x.block_off.view(np.int32))
    out_cap = x.total + 64
    wire, woff, st = codec.write_frames(dblob, dboff, to_dev(x.stream_id.view(np.int32)), to_dev(x.max_frame.view(np.int32)),
                                        out_blob=torch.empty(out_cap, dtype=torch.uint8, device="cuda"), sync=True)
    assert np.array_equal(woff.cpu().numpy().view(np.uint32), x.wire_off) and not st.cpu().numpy().any()
    # the connections: their blocks' frames end to end
    first = [conn_of.index(c) for c in range(nconn)] + [n]
    coff = x.wire_off[first]
    conns = np.zeros(nconn, fc.FCONN_DTYPE)
    conns["max_frame_size"] = [items[first[c]][2] for c in range(nconn)]
    dconns = to_dev(conns.view(np.uint8).reshape(-1))
    blocks, cb, fo, fl, cf, oo, ol, co = codec.scan_frames(wire[: x.total], to_dev(coff.view(np.int32)), dconns, sync=True)
    nb, nf = int(cb[nconn].item()), int(cf[nconn].item())
    assert nb == n and int(co[nconn].item()) == 0
    assert not dconns.cpu().numpy().view(fc.FCONN_DTYPE)["error"].any()
    rec = blocks[: 16 * nb].cpu().numpy().view(fc.FBLOCK_DTYPE)
    assert np.array_equal(rec["stream_id"], x.stream_id) and np.array_equal(rec["conn"], np.asarray(conn_of, np.uint32))
    assert np.array_equal(rec["nfrag"], [wc.frame_count(len(b), m) for b, _, m in items])
    blk, boff = codec.frame_blocks(wire[: x.total], fo[:nf], fl[:nf], blocks, nblocks=nb, sync=True)
    assert np.array_equal(boff.cpu().numpy().view(np.uint32), x.block_off)
    assert np.array_equal(blk.cpu().numpy()[: x.blob.size], x.blob)
    # on to header lists for the first connections (the chain of tests/test_gpu_frames_scan.py)
    sub = 6
    nb2 = first[sub]
    fields, foff, so, se, soff, _ = codec.scan_blocks(blk, boff[: nb2 + 1].contiguous(), sync=True)
    ns, nfields = int(soff[nb2].item()), int(foff[nb2].item())
    out, so_off, so_len, _, sst = codec.decode_strings(blk, so[:ns], se[:ns], sync=True)
    g3 = [ctypes.c_uint32(0) for _ in range(3)]
    assert _lib.lib().hpk_test_blkapply_geometry(*[ctypes.byref(g) for g in g3]) == _lib.HPK_E_OK
    per = g3[0].value
    text, _ = batch.static_table()
    tabs = np.zeros(sub, batch.DTAB_DTYPE)
    tabs["ent"] = np.arange(sub) * per
    tabs["cap"] = per
    tabs["max_size"] = 4096
    tabs["max_allowed"] = _lib.HPK_DTAB_NO_LIMIT
    headers, results = codec.apply_blocks(fields[: 16 * nfields], foff, so_off, so_len, sst, ns, len(text), 0, cb[: sub + 1].contiguous(),
                                          torch.arange(nb2, dtype=torch.int32, device="cuda"), to_dev(tabs.view(np.uint8).reshape(-1)),
                                          torch.zeros(16 * per * sub, dtype=torch.uint8, device="cuda"), sync=True)
    arena = text + out.cpu().numpy().tobytes()
    res = results.cpu().numpy().view(batch.RESULT_DTYPE)[:nb2]
    hdr = headers.cpu().numpy().view(batch.HEADER_DTYPE)
    assert not res["error"].any()
    got = [[(arena[h["name_off"] : h["name_off"] + h["name_len"]], arena[h["value_off"] : h["value_off"] + h["value_len"]])
            for h in hdr[res[b]["first_header"] : res[b]["first_header"] + res[b]["n_headers"]]] for b in range(nb2)]
    assert got == [hl for _, lists in stories[:sub] for hl in lists]
