"""The header-block scan on the GPU (hpk_scan_blocks), record for record: no tolerance. The expected result is
blocks_scan_cases.expected_batch(): ref_scan block by block, which test_blocks_scan_cases.py pins to
hpack_ref.Decoder; never the code under test.

One checker serves every case: the field records and the string windows go into views of canary-filled buffers with
guards behind them, field_off, str_blk_off and status are prefilled with values the call never writes; afterwards
the arrays are the expected ones, the records and windows below min(total, capacity) are the expected ones, and
the canary is intact at and past that point."""

import ctypes

import numpy as np
import pytest

import blocks_scan_cases as bc
from hpk_util import hpack_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CANARY = 0xA5
CANARY32 = np.int32(-0x5A5A5A5B)  # 0xA5A5A5A5
GUARD = 4096
PRE_OFF, PRE_ST = -3, 9
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
def wg_blocks():
    from loona_amd import _lib

    w = ctypes.c_uint32(0)
    assert _lib.lib().hpk_test_blkscan_geometry(ctypes.byref(w)) == _lib.HPK_E_OK
    assert w.value >= 64
    return w.value


@pytest.fixture(scope="module")
def placed_blocks():
    return [b for _, b, _ in bc.placed()]


@pytest.fixture(scope="module")
def interop():
    blocks = bc.interop_blocks()
    return blocks, bc.expected_batch(blocks)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(codec, x, in_shift=0, fields_cap=None, strs_cap=None, sync=True, raises=None):
    """scan_blocks on batch x with the blob in_shift bytes off a 256-byte boundary -> (fields, field_off, str_off,
    str_end, str_blk_off, status, intact): the lists as far as their capacities reach"""
    n = len(x.block_off) - 1
    fcap = x.blob.size if fields_cap is None else fields_cap
    scap = x.blob.size if strs_cap is None else strs_cap
    src = np.zeros(in_shift + x.blob.size + 1, np.uint8)
    src[in_shift : in_shift + x.blob.size] = x.blob
    dblob = to_dev(src)[in_shift : in_shift + x.blob.size]
    boff = to_dev(x.block_off.view(np.int32))
    fbig = torch.full((16 * fcap + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    sbig = torch.full((scap + GUARD,), int(CANARY32), dtype=torch.int32, device="cuda")
    ebig = torch.full((scap + GUARD,), int(CANARY32), dtype=torch.int32, device="cuda")
    foff = torch.full((n + 1,), PRE_OFF, dtype=torch.int32, device="cuda")
    soff = torch.full((n + 1,), PRE_OFF, dtype=torch.int32, device="cuda")
    st = torch.full((max(n, 1),), PRE_ST, dtype=torch.uint8, device="cuda")
    kw = dict(fields=fbig[: 16 * fcap], field_off=foff, str_off=sbig[:scap], str_end=ebig[:scap], str_blk_off=soff, status=st)
    if raises is None:
        codec.scan_blocks(dblob, boff, sync=sync, **kw)
        if not sync:
            codec.check()
    else:
        with pytest.raises(RuntimeError, match=raises):
            codec.scan_blocks(dblob, boff, sync=True, **kw)
    torch.cuda.synchronize()
    u = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    f, s, e = fbig.cpu().numpy(), sbig.cpu().numpy(), ebig.cpu().numpy()
    return f, u(foff), s, e, u(soff), st[:n].cpu().numpy(), (fcap, scap)


def compare(what, x, got):
    f, foff, s, e, soff, st, (fcap, scap) = got
    assert np.array_equal(foff, x.field_off), f"{what}: field_off"
    assert np.array_equal(soff, x.str_blk_off), f"{what}: str_blk_off"
    assert not st.any(), f"{what}: status"
    nf, ns = min(len(x.fields), fcap), min(len(x.str_off), scap)
    gf = f[: 16 * nf].view(bc.FIELD_DTYPE)
    if not np.array_equal(gf, x.fields[:nf]):
        i = int(np.nonzero(gf != x.fields[:nf])[0][0])
        b = int(np.searchsorted(x.field_off, i, "right")) - 1
        raise AssertionError(f"{what}: field {i} (block {b}): {gf[i]} for {x.fields[i]}")
    assert np.array_equal(s[:ns].view(np.uint32), x.str_off[:ns]), f"{what}: str_off"
    assert np.array_equal(e[:ns].view(np.uint32), x.str_end[:ns]), f"{what}: str_end"
    assert (f[16 * nf :] == CANARY).all(), f"{what}: records at or past min(total, fields_cap) were written"
    assert (s[ns:] == CANARY32).all() and (e[ns:] == CANARY32).all(), f"{what}: windows at or past min(total, strs_cap) were written"


def compare_host(what, x, got):
    f, foff, so, se, soff, st = got
    assert np.array_equal(foff, x.field_off) and np.array_equal(soff, x.str_blk_off), f"{what}: offsets"
    assert not st.any(), f"{what}: status"
    assert np.array_equal(f, x.fields), f"{what}: fields"
    assert np.array_equal(so, x.str_off) and np.array_equal(se, x.str_end), f"{what}: windows"


def test_placed_cases_device_and_host(codec, placed_blocks):
    x = bc.expected_batch(placed_blocks)
    assert {int(k) for k in x.fields["err_stage"][x.fields["err"] != 0]} == {0, 1, 2}
    compare("placed, device", x, run(codec, x))
    compare_host("placed, host", x, codec.scan_blocks_host(x.blob, x.block_off))


def test_interop_corpus_one_call(codec, interop):
    blocks, x = interop
    assert len(blocks) > 16000
    compare("interop, device", x, run(codec, x))
    compare_host("interop, host", x, codec.scan_blocks_host(x.blob, x.block_off))


@pytest.mark.parametrize("where", ["wg-1", "wg", "wg+1", "4095", "4096", "4097"])
def test_block_counts_at_the_cuts(codec, wg_blocks, interop, where):
    """block counts on each side of a workgroup's blocks and of the scan's tile (4,096 elements over n + 1)"""
    n = {"wg-1": wg_blocks - 1, "wg": wg_blocks, "wg+1": wg_blocks + 1}.get(where) or int(where)
    blocks = interop[0][100 : 100 + n]
    x = bc.expected_batch(blocks)
    compare(f"{n} blocks", x, run(codec, x))


def test_one_block_of_many_fields_among_small_ones(codec, placed_blocks):
    """one block of 5,000 one-octet fields (and one of 2,100 two-string literals) among small blocks: field_off
    and str_blk_off step by more than a scan tile inside the batch"""
    big = bytes([0x82 + (i % 60) for i in range(5000)])
    lits = b"\x00\x01a\x01b" * 2100
    blocks = placed_blocks[:40] + [big] + placed_blocks[40:90] + [lits] + placed_blocks[90:]
    x = bc.expected_batch(blocks)
    assert x.field_off[41] - x.field_off[40] == 5000 and x.str_blk_off[92] - x.str_blk_off[91] == 4200
    compare("big block", x, run(codec, x))


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_blob_misalignment(codec, placed_blocks, interop, shift):
    x = bc.expected_batch(placed_blocks + interop[0][:600], base=shift)
    compare(f"shift {shift}", x, run(codec, x, in_shift=shift))
    compare(f"shift {shift}, blocks from offset {shift}", x, run(codec, x, in_shift=(4 - shift) % 4))


@pytest.mark.parametrize("which", ["fields", "strs"])
@pytest.mark.parametrize("delta", ["zero", -1, 0, 1])
def test_capacities(codec, placed_blocks, interop, which, delta):
    x = bc.expected_batch(placed_blocks + interop[0][:300])
    total = len(x.fields) if which == "fields" else len(x.str_off)
    cap = 0 if delta == "zero" else total + delta
    kw = {"fields_cap" if which == "fields" else "strs_cap": cap}
    short = cap < total
    compare(f"{which} cap {cap}", x, run(codec, x, raises="-2" if short else None, **kw))
    compare(f"{which} cap {cap}, async", x, run(codec, x, sync=False, **kw))  # (an async call cannot say NOSPACE)
    if short:
        with pytest.raises(RuntimeError, match="-2"):
            codec.scan_blocks_host(x.blob, x.block_off, **kw)
    else:
        compare_host(f"{which} cap {cap}, host", x, codec.scan_blocks_host(x.blob, x.block_off, **kw))


def test_host_capacity_writes_only_below_it(codec, placed_blocks):
    """host pointers: exactly the written parts come back (numpy canaries behind the capacities)"""
    from loona_amd import _lib

    x = bc.expected_batch(placed_blocks)
    n = len(x.block_off) - 1
    fcap, scap = len(x.fields) - 7, len(x.str_off) - 3
    f = np.full(16 * len(x.fields) + 64, CANARY, np.uint8)
    so = np.full(len(x.str_off) + 16, 0xA5A5A5A5, np.uint32)
    se = so.copy()
    foff, soff, st = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32), np.zeros(n, np.uint8)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    rc = _lib.lib().hpk_scan_blocks(codec._h, p(x.blob), x.blob.size, p(x.block_off), n, p(f), fcap, p(foff), p(so), p(se), scap,
                                    p(soff), p(st), _lib.HPK_PTR_HOST)
    assert rc == _lib.HPK_E_NOSPACE
    assert np.array_equal(foff, x.field_off) and np.array_equal(soff, x.str_blk_off) and not st.any()
    assert np.array_equal(f[: 16 * fcap].view(bc.FIELD_DTYPE), x.fields[:fcap]) and (f[16 * fcap :] == CANARY).all()
    assert np.array_equal(so[:scap], x.str_off[:scap]) and (so[scap:] == 0xA5A5A5A5).all()
    assert np.array_equal(se[:scap], x.str_end[:scap]) and (se[scap:] == 0xA5A5A5A5).all()


@pytest.mark.parametrize("kind", ["decreasing", "past cap"])
def test_bad_offsets(codec, placed_blocks, kind):
    """a block whose own offsets decrease, or whose end passes cap, is void (HPK_BAD_OFFSETS, 0 fields, 0 strings,
    the sticky flag); every other block is scanned as it lies"""
    from loona_amd import _lib

    blocks = placed_blocks[:64]
    x = bc.expected_batch(blocks)
    boff = x.block_off.astype(np.int64)
    if kind == "decreasing":
        k = 20  # block 20 ends before it starts; block 21 starts earlier, inside block 20's bytes, and is read as it lies
        boff[k + 1] = boff[k] - 2
        void = [k]
        in_cap = None
    else:
        in_cap = int(boff[-2])  # the blob's capacity ends where the last block starts
        void = [b for b in range(64) if boff[b + 1] > in_cap]
        assert void == [63] and len(blocks[63]) > 0
    want_blocks = []
    for b in range(64):
        lo, hi = int(boff[b]), int(boff[b + 1])
        want_blocks.append(b"" if b in void else x.blob[lo:hi].tobytes())
    f, foff, s, e, soff, st, _ = _bad_run(codec, x, boff, in_cap)
    assert [int(v) for v in np.nonzero(st)[0]] == void and (st[void] == BAD_OFFSETS).all()
    nf = np.diff(foff.astype(np.int64))
    ns = np.diff(soff.astype(np.int64))
    for b in range(64):
        fields, strings = bc.ref_scan(want_blocks[b])
        assert nf[b] == len(fields) and ns[b] == len(strings), b
        got = f[16 * int(foff[b]) : 16 * int(foff[b + 1])].view(bc.FIELD_DTYPE)
        assert [int(v) for v in got["at"]] == [int(boff[b]) + fl.at for fl in fields], b
        assert [int(v) for v in got["err"]] == [fl.err for fl in fields], b
    # the host form checks the offsets before anything is copied
    with pytest.raises(RuntimeError, match="-1"):
        codec.scan_blocks_host(x.blob[: (x.blob.size if in_cap is None else in_cap)], boff.astype(np.uint32))
    # cap above HPK_MAX_OFFSET
    z = torch.zeros(64, dtype=torch.int32, device="cuda")
    rc = _lib.lib().hpk_scan_blocks(codec._h, ctypes.c_void_p(z.data_ptr()), _lib.HPK_MAX_OFFSET + 1, ctypes.c_void_p(z.data_ptr()), 0,
                                    None, 0, ctypes.c_void_p(z.data_ptr()), None, None, 0, ctypes.c_void_p(z.data_ptr()), None,
                                    _lib.HPK_PTR_DEVICE)
    assert rc == _lib.HPK_E_INVAL


def _bad_run(codec, x, boff, in_cap):
    """an async call with bad offsets: the outputs, then the sticky flag through check()"""
    n = len(boff) - 1
    cap = x.blob.size if in_cap is None else in_cap
    dblob = to_dev(x.blob)[:cap]
    dboff = to_dev(boff.astype(np.uint32).view(np.int32))
    out = codec.scan_blocks(dblob, dboff, sync=False)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="HPK_BAD_OFFSETS"):
        codec.check()
    codec.check()  # (read and cleared)
    with pytest.raises(RuntimeError, match="HPK_BAD_OFFSETS"):  # a synchronous call says so itself
        codec.scan_blocks(dblob, dboff, sync=True)
    fields, foff, so, se, soff, st = out
    u = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    return fields.cpu().numpy(), u(foff), u(so), u(se), u(soff), st[:n].cpu().numpy(), None


def test_no_blocks(codec):
    x = bc.expected_batch([])
    f, foff, s, e, soff, st, _ = run(codec, x)
    assert list(foff) == [0] and list(soff) == [0] and (f == CANARY).all()
    got = codec.scan_blocks_host(x.blob, x.block_off)
    assert list(got[1]) == [0] and list(got[4]) == [0] and len(got[0]) == 0
    # blocks of no bytes
    y = bc.expected_batch([b"", b"", b""])
    compare("three empty blocks", y, run(codec, y))


def test_async_then_check(codec, interop):
    x = bc.expected_batch(interop[0][:2000])
    compare("async", x, run(codec, x, sync=False))


def test_scan_feeds_decode_strings(codec, placed_blocks, interop):
    """str_off / str_end as they stand into decode_strings: every listed string equals hpack_ref.decode_string on
    its window, Huffman statuses included"""
    blocks = placed_blocks + [w for s in bc.corrupted_stories() for w in s] + bc.random_blocks(n=600) + interop[0][::16]
    x = bc.expected_batch(blocks)
    dblob = to_dev(x.blob)
    fields, foff, so, se, soff, st = codec.scan_blocks(dblob, to_dev(x.block_off.view(np.int32)), sync=True)
    ns = int(soff[-1].item())
    assert ns == len(x.str_off) > 5000
    out, oo, ol, co, sst = codec.decode_strings(dblob, so[:ns], se[:ns], sync=True)
    out, oo, ol, co, sst = out.cpu().numpy(), oo.cpu().numpy().view(np.uint32), ol.cpu().numpy(), co.cpu().numpy(), sst.cpu().numpy()
    raw = x.blob.tobytes()
    bad_huff = 0
    for i in range(ns):
        a, e = int(x.str_off[i]), int(x.str_end[i])
        assert co[i] == e - a, i
        try:
            want, consumed = hpack_ref.decode_string(raw[a:e])
        except hpack_ref.DecoderError as err:
            assert err.detail[0] == "HuffmanDecoderError" and sst[i] == err.detail[1], i
            bad_huff += 1
            continue
        assert consumed == e - a and sst[i] == 0 and ol[i] == len(want), i
        assert out[int(oo[i]) : int(oo[i]) + int(ol[i])].tobytes() == want, i
    assert bad_huff >= 3
