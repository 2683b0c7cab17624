"""The packed output form on the GPU: hpk_decode_batch_packed, hpk_pack_batch, shard.compact(codec=...).

A packed decode must give what HuffmanDecoder::decode (huffman.rs:98, 160) would have produced for each
literal, concatenated: out_off the exclusive sum of out_len, the bytes end to end with no gap, nothing
written at or past out_off[n] nor outside the caller's capacity. The expected result is always built from
the oracle (oracle_decode_batch): its valid bytes concatenated, the exclusive sum of its out_len, its
statuses. Inputs with chosen DECODED lengths are plaintexts run through oracle_encode_batch. The edge cases
are placed relative to the pack kernel's own geometry (hpk_test_pack_geometry): T = the bytes of a
destination tile, L = the literals a workgroup stages in LDS at a time."""

import ctypes

import numpy as np
import pytest

from hpk_util import interop_literals, load, oracle_decode, oracle_decode_batch, oracle_encode_batch, pack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CANARY = 0xA5
GUARD = 4096


@pytest.fixture(scope="module", params=["fill", "wave"])
def codec(request):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU)")
    from loona_amd import HuffmanCodec

    c = HuffmanCodec(0, stream=torch.cuda.current_stream())
    c.set_decode_kernel(request.param)
    yield c
    c.close()


@pytest.fixture(scope="module")
def geo():
    from loona_amd import _lib

    t, l = ctypes.c_uint32(0), ctypes.c_uint32(0)
    assert _lib.lib().hpk_test_pack_geometry(ctypes.byref(t), ctypes.byref(l)) == 0
    assert t.value % 16 == 0 and t.value and l.value
    return t.value, l.value


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gather(out, starts, lens):
    """the bytes out[starts[i] : starts[i] + lens[i]] laid end to end, and their exclusive sum"""
    lens = np.asarray(lens, np.int64)
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    tot = int(off[-1])
    if tot == 0:
        return np.zeros(0, np.uint8), off
    idx = np.repeat(np.asarray(starts, np.int64)[: len(lens)] - off[:-1], lens) + np.arange(tot)
    return out[idx], off


def expected(blob, off):
    """(flat bytes, out_off int64 [n+1], out_len, status) from the oracle"""
    out, oo, ol, st = oracle_decode_batch(blob, off)
    flat, eoff = gather(out, oo, ol)
    return flat, eoff, ol, st


def encode_plain(lens, seed=0):
    """Encoded literals whose decoded lengths are exactly `lens` (text bytes through the oracle's encoder)."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    plain = rng.integers(0x20, 0x7F, size=max(int(off[-1]), 1), dtype=np.uint8)[: int(off[-1])]
    eb, eo, el, est = oracle_encode_batch(plain, off.astype(np.uint32))
    assert not est.any()
    blob, eoff = gather(eb, eo, el)
    return blob, eoff.astype(np.uint32)


def run_packed(codec, blob, off, in_shift=0, out_shift=0, cap=None, sync=True, raises=None):
    """decode_packed into a view of `cap` bytes (default: the expected total) `out_shift` bytes into a
    canary-filled buffer -> (view bytes, out_off, out_len, status, canary intact outside the view)"""
    blob = np.ascontiguousarray(blob, np.uint8)
    n = len(off) - 1
    pad = np.zeros(blob.size + in_shift + 1, np.uint8)
    pad[in_shift : in_shift + blob.size] = blob
    dblob = to_dev(pad)[in_shift : in_shift + max(blob.size, 1)]
    doff = to_dev(np.asarray(off, np.int64).astype(np.uint32).view(np.int32))
    if cap is None:
        cap = int(expected(blob, np.asarray(off, np.uint32))[1][-1])
    big = torch.full((GUARD + out_shift + cap + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    view = big[GUARD + out_shift : GUARD + out_shift + cap]
    oo = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
    ol = torch.full((max(n, 1),), 7, dtype=torch.int32, device="cuda")
    st = torch.full((max(n, 1),), 9, dtype=torch.uint8, device="cuda")
    if raises is None:
        codec.decode_packed(dblob, doff, out_blob=view, out_off=oo, out_len=ol, status=st, sync=sync)
    else:
        with pytest.raises(RuntimeError, match=raises):
            codec.decode_packed(dblob, doff, out_blob=view, out_off=oo, out_len=ol, status=st, sync=True)
    torch.cuda.synchronize()
    g = big.cpu().numpy()
    return (g[GUARD + out_shift : GUARD + out_shift + cap], oo.cpu().numpy().view(np.uint32).astype(np.int64),
            ol[:n].cpu().numpy().view(np.uint32), st[:n].cpu().numpy(), g[: GUARD + out_shift], g[GUARD + out_shift + cap :])


def check_packed(codec, blob, off, what, in_shift=0, out_shift=0, cap=None, raises=None, exp=None):
    flat, eoff, el, est = exp if exp is not None else expected(blob, off)  # (exp: the oracle's result, made once)
    total = int(eoff[-1])
    got, oo, ol, st, pre, post = run_packed(codec, blob, off, in_shift, out_shift, total if cap is None else cap,
                                            raises=raises)
    assert np.array_equal(st, est), f"{what}: status"
    assert np.array_equal(ol, el), f"{what}: out_len"
    assert np.array_equal(oo, eoff), f"{what}: out_off is not the exclusive sum of the oracle's out_len"
    k = min(total, len(got))
    if not np.array_equal(got[:k], flat[:k]):
        first = int(np.nonzero(got[:k] != flat[:k])[0][0])
        raise AssertionError(f"{what}: bytes differ first at {first} (literal {int(np.searchsorted(eoff, first, 'right')) - 1})")
    assert (got[k:] == CANARY).all(), f"{what}: bytes at or past out_off[n] were written"
    assert (pre == CANARY).all() and (post == CANARY).all(), f"{what}: bytes outside the output view were written"
    return total


def test_reference_vectors(codec):
    """The KATs, the RFC 7541 App. C literals and the error vectors in one batch: error literals keep the
    bytes decoded before their error, in place in the stream."""
    lits = [bytes.fromhex(k["in"]) for k in load("kat.json")]
    lits += [bytes.fromhex(x["in"]) for x in load("rfc7541_blocks.json")["huffman_literals"]]
    vecs = load("error_vectors.json")["vectors"]
    lits += [bytes.fromhex(v["in"]) for v in vecs]
    blob, off = pack(lits)
    check_packed(codec, blob, off, "reference vectors")
    _, _, _, st, _, _ = run_packed(codec, blob, off)
    assert [int(s) for s in st[-len(vecs) :]] == [v["status"] for v in vecs]


_interop_exp = None


def _interop_expected(blob, off):
    global _interop_exp
    if _interop_exp is None:
        _interop_exp = expected(blob, off)
    return _interop_exp


@pytest.mark.parametrize("in_shift", [0, 3])
def test_interop_corpus_misaligned(codec, in_shift):
    lits = interop_literals()
    blob, off = pack(lits)
    exp = _interop_expected(blob, off)
    for out_shift in (0, 1, 5, 15):
        check_packed(codec, blob, off, f"interop (in +{in_shift}, out +{out_shift})", in_shift, out_shift, exp=exp)


def _shorts(rng, k):
    return [int(x) for x in rng.integers(0, 40, k)]


def _exact_total(rng, tot):
    v, left = [], tot
    while left:
        x = min(left, int(rng.integers(1, 200)))
        v.append(x)
        left -= x
    return v


GEOMETRY = ["quarter", "long_mid_tile", "empties", "one_byte", "total_2T", "total_2T-1", "total_2T+1", "total_17",
            "all_empty", "n1", "n0"]


@pytest.mark.parametrize("case", GEOMETRY)
def test_tile_geometry(codec, geo, case):
    """Literal boundaries on the tile edges, a literal over several tiles from the middle of one, more
    literals under one tile than the LDS stage holds (empty and one-byte runs), exact totals around the
    tile size, an all-empty batch, one literal and none; short literals before and after each special run."""
    T, L = geo
    rng = np.random.default_rng(11)
    a, z = _shorts(rng, 25), _shorts(rng, 25)
    lens = {
        "quarter": a + [T // 4] * 13 + z,
        "long_mid_tile": a + [3 * T + 5] + z,
        "empties": a + [0] * (L + 1000) + z,
        "one_byte": a + [1] * (2 * L) + z,
        "total_2T": _exact_total(rng, 2 * T),
        "total_2T-1": _exact_total(rng, 2 * T - 1),
        "total_2T+1": _exact_total(rng, 2 * T + 1),
        "total_17": _exact_total(rng, 17),
        "all_empty": [0] * 300,
        "n1": [37],
        "n0": [],
    }[case]
    blob, off = encode_plain(lens, seed=3)
    total = check_packed(codec, blob, off, case, out_shift=0)
    assert total == sum(lens)
    check_packed(codec, blob, off, case + " (out +7)", in_shift=5, out_shift=7)
    if case == "quarter":  # the T/4 literals exactly on the tile edges of an aligned blob
        blob, off = encode_plain([T // 4] * 12, seed=4)
        check_packed(codec, blob, off, "quarter tiles on the edges")


def _zipf_batch():
    rng = np.random.default_rng(21)
    lens = np.minimum(rng.zipf(1.3, 3000) - 1, 4096).tolist()
    lens.insert(1500, 256 * 1024)
    return encode_plain(lens, seed=5)


def _random_bytes_batch():
    rng = np.random.default_rng(22)
    lits = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, 71, 20000)]
    return pack(lits)


@pytest.mark.parametrize("kind", ["zipf_and_huge", "random_bytes"])
def test_mixed_lengths(codec, kind):
    """Zipf lengths up to 4 KiB plus one 256 KiB literal (the long and the huge phase feed the pack), and 20k
    literals of 0-70 random bytes (mostly padding errors, their partial bytes kept)."""
    blob, off = _zipf_batch() if kind == "zipf_and_huge" else _random_bytes_batch()
    check_packed(codec, blob, off, kind, out_shift=9)
    if kind == "random_bytes":
        assert expected(blob, off)[3].any()


def test_capacity(codec, geo):
    """out_cap == total leaves every canary byte; a smaller capacity makes the synchronous call fail with
    HPK_E_NOSPACE (-2) with out_off, out_len and status complete, the bytes below out_cap right and
    nothing else written."""
    T, _ = geo
    rng = np.random.default_rng(31)
    blob, off = encode_plain(rng.integers(0, 90, 600).tolist(), seed=6)
    total = check_packed(codec, blob, off, "cap == total", out_shift=3)
    assert total > T + 3
    for cap in (total - 1, T + 3, 0):
        check_packed(codec, blob, off, f"cap {cap}", out_shift=3, cap=cap, raises=r"hpk_decode_batch_packed failed \(-2\)")


def test_bad_offsets(codec):
    """One decreasing in_off in the middle of 10k literals: HPK_E_INVAL (-1), every status the oracle's or
    HPK_BAD_OFFSETS, out_off the exclusive sum of out_len, the canary intact, and the codec good afterwards."""
    from loona_amd import _lib, synth

    w = synth.config2(n=10000, seed=5)
    io = w.enc_off.astype(np.int64).copy()
    j = 5000
    io[j] = io[j + 1] + 3  # literal j decreases; literal j - 1 now runs 3 bytes into literal j + 1
    want = oracle_decode_batch(w.enc_blob, w.enc_off)
    cap = int(want[2].astype(np.int64).sum()) + 4096
    got, oo, ol, st, pre, post = run_packed(codec, w.enc_blob, io, cap=cap, raises=r"hpk_decode_batch_packed failed \(-1\)")
    bad = st == _lib.HPK_BAD_OFFSETS
    assert bad[j]
    ws = want[3].copy()
    ws[j - 1] = oracle_decode(w.enc_blob[io[j - 1] : io[j]].tobytes())[0]
    assert ((st == ws) | bad).all()
    assert (ol[bad] == 0).all()
    eoff = np.concatenate([[0], np.cumsum(ol.astype(np.int64))])
    assert np.array_equal(oo, eoff)
    assert (got[int(eoff[-1]) :] == CANARY).all() and (pre == CANARY).all() and (post == CANARY).all()
    codec.check()  # the failing synchronous call cleared the sticky flag
    check_packed(codec, w.enc_blob, w.enc_off, "after bad offsets")


def test_streams_and_scratch_reuse(codec):
    """Two different batches in flight on two streams through one codec (their scratch is per stream), then
    a large call followed by a small one on the same stream (the grown scratch reused)."""
    from loona_amd import HuffmanCodec, synth

    rng = np.random.default_rng(41)
    b1 = encode_plain(rng.integers(0, 120, 30000).tolist(), seed=7)
    b2 = encode_plain(rng.integers(0, 60, 50000).tolist(), seed=8)
    c = HuffmanCodec(0)  # follows torch's current stream at each call
    c.set_decode_kernel("auto")
    try:
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        d = [(to_dev(b), to_dev(o.view(np.int32))) for b, o in (b1, b2)]
        torch.cuda.synchronize()
        res = []
        for _ in range(2):
            for s, (db, do) in zip((s1, s2), d):
                with torch.cuda.stream(s):
                    res.append(c.decode_packed(db, do))
        for s in (s1, s2):
            s.synchronize()
        c.check()
        for k, (pb, po, pl, pst) in enumerate(res):
            flat, eoff, el, est = expected(*((b1, b2)[k % 2]))
            n = len(el)
            assert np.array_equal(po.cpu().numpy().view(np.uint32).astype(np.int64), eoff)
            assert np.array_equal(pl[:n].cpu().numpy().view(np.uint32), el) and np.array_equal(pst[:n].cpu().numpy(), est)
            assert np.array_equal(pb.cpu().numpy()[: len(flat)], flat), f"two streams: call {k}"
    finally:
        c.close()
    w = synth.config2(n=100000, seed=9)
    check_packed(codec, w.enc_blob, w.enc_off, "100k literals")
    lits = [w.enc_blob[w.enc_off[i] : w.enc_off[i + 1]].tobytes() for i in range(100)]
    check_packed(codec, *pack(lits), "100 literals after 100k")


def test_pack_alone(codec):
    """hpk_pack_batch: 50k pieces whose starts are a random permutation of gapped regions, some empty and
    some 40 KiB long, equal a numpy gather; a piece passing src_cap counts 0 bytes and raises the sticky
    error, with nothing written out of range."""
    rng = np.random.default_rng(51)
    n = 50000
    lens = rng.integers(0, 64, n).astype(np.int64)
    lens[rng.integers(0, n, 2000)] = 0
    lens[rng.integers(0, n, 6)] = 40 * 1024
    order = rng.permutation(n)
    gaps = rng.integers(0, 9, n)
    starts = np.zeros(n, np.int64)
    at = 5
    pos = np.cumsum(np.concatenate([[at], (lens[order] + gaps)[:-1]]))
    starts[order] = pos
    src_cap = int(pos[-1] + lens[order[-1]]) + 11
    src = rng.integers(0, 256, src_cap, dtype=np.uint8)
    flat, eoff = gather(src, starts, lens)
    total = int(eoff[-1])
    dsrc = to_dev(np.concatenate([np.zeros(3, np.uint8), src]))[3:]  # (a misaligned base)
    dso, dsl = to_dev(starts.astype(np.uint32).view(np.int32)), to_dev(lens.astype(np.uint32).view(np.int32))
    big = torch.full((GUARD + 5 + total + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    view = big[GUARD + 5 : GUARD + 5 + total]
    _, doff = codec.pack(dsrc, dso, dsl, dst_blob=view, sync=True)
    g = big.cpu().numpy()
    assert np.array_equal(doff.cpu().numpy().view(np.uint32).astype(np.int64), eoff)
    assert np.array_equal(g[GUARD + 5 : GUARD + 5 + total], flat)
    assert (g[: GUARD + 5] == CANARY).all() and (g[GUARD + 5 + total :] == CANARY).all()
    # allocating form: cut to the total
    pb, _ = codec.pack(dsrc, dso, dsl, sync=True)
    assert np.array_equal(pb.cpu().numpy(), flat)
    # one piece passes src_cap
    k = int(order[n // 2])
    bad_starts = starts.copy()
    bad_starts[k] = src_cap - 1
    lens2 = lens.copy()
    lens2[k] = 2
    want_lens = lens2.copy()
    want_lens[k] = 0
    flat2, eoff2 = gather(src, bad_starts, want_lens)
    big.fill_(CANARY)
    doff.fill_(-1)
    with pytest.raises(RuntimeError, match=r"hpk_pack_batch failed \(-1\)"):
        codec.pack(dsrc, to_dev(bad_starts.astype(np.uint32).view(np.int32)), to_dev(lens2.astype(np.uint32).view(np.int32)),
                   dst_blob=view, dst_off=doff, sync=True)
    g = big.cpu().numpy()
    assert np.array_equal(doff.cpu().numpy().view(np.uint32).astype(np.int64), eoff2)
    t2 = int(eoff2[-1])
    assert np.array_equal(g[GUARD + 5 : GUARD + 5 + t2], flat2)
    assert (g[: GUARD + 5] == CANARY).all() and (g[GUARD + 5 + t2 :] == CANARY).all()
    codec.check()


def _pack_into_view(codec, src, starts, lens, cap, shift=5, raises=None):
    """codec.pack (synchronous) of host pieces into a view of `cap` bytes between canaries ->
    (dst_off as int64, the view's bytes, canaries intact)"""
    dsrc = to_dev(src)
    dso, dsl = to_dev(np.asarray(starts, np.uint32).view(np.int32)), to_dev(np.asarray(lens, np.uint32).view(np.int32))
    big = torch.full((GUARD + shift + cap + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    view = big[GUARD + shift : GUARD + shift + cap]
    doff = torch.full((len(lens) + 1,), -1, dtype=torch.int32, device="cuda")
    if raises is None:
        codec.pack(dsrc, dso, dsl, dst_blob=view, dst_off=doff, sync=True)
    else:
        with pytest.raises(RuntimeError, match=raises):
            codec.pack(dsrc, dso, dsl, dst_blob=view, dst_off=doff, sync=True)
    torch.cuda.synchronize()
    g = big.cpu().numpy()
    intact = bool((g[: GUARD + shift] == CANARY).all() and (g[GUARD + shift + cap :] == CANARY).all())
    return doff.cpu().numpy().view(np.uint32).astype(np.int64), g[GUARD + shift : GUARD + shift + cap], intact


@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097, 16_781_313])
def test_length_scan(codec, request, n):
    """hpk_pack_batch's dst_off across the scan's tile boundary (4,096 pieces) and past one workgroup of tile
    sums (16,777,216 pieces): the numpy exclusive sum. Small sizes: lengths 0-40 with some zeros, gapped
    sources, the bytes a numpy gather, the canaries intact. The large size: lengths 0-3, every piece at one
    small offset of a small source, dst_off only."""
    rng = np.random.default_rng(n + 61)
    if n > 4097:
        if request.node.callspec.params["codec"] != "wave":
            pytest.skip("one kernel variant is enough for the large size")
        lens = rng.integers(0, 4, n).astype(np.int64)
        eoff = np.zeros(n + 1, np.int64)
        np.cumsum(lens, out=eoff[1:])
        src = to_dev(rng.integers(0, 256, 16, dtype=np.uint8))
        dso = torch.full((n,), 5, dtype=torch.int32, device="cuda")
        dst = torch.empty(int(eoff[-1]), dtype=torch.uint8, device="cuda")
        _, doff = codec.pack(src, dso, to_dev(lens.astype(np.int32)), dst_blob=dst, sync=True)
        got = doff.cpu().numpy().view(np.uint32).astype(np.int64)
        assert np.array_equal(got, eoff), np.nonzero(got != eoff)[0][:5]
        return
    lens = rng.integers(0, 41, n).astype(np.int64)
    if n:
        lens[rng.integers(0, n, max(n // 50, 1))] = 0
    starts = 5 + np.concatenate([[0], np.cumsum(lens + rng.integers(0, 9, n))[:-1]]).astype(np.int64)[:n]
    src = rng.integers(0, 256, int(starts[-1] + lens[-1]) + 11 if n else 11, dtype=np.uint8)
    flat, eoff = gather(src, starts, lens)
    got, out, intact = _pack_into_view(codec, src, starts, lens, int(eoff[-1]))
    assert np.array_equal(got, eoff), np.nonzero(got != eoff)[0][:5]
    assert np.array_equal(out, flat)
    assert intact


@pytest.mark.parametrize("n", [4095, 4100])
def test_length_scan_total_boundary(codec, n):
    """Both sides of the 64-bit tile sums' limit, every piece the same 2^20 source bytes into a 4,096-byte
    destination. 4,095 pieces total 4,293,918,720 <= HPK_MAX_OFFSET: dst_off exact, the first 4,096 bytes
    packed, HPK_E_NOSPACE (-2). 4,100 pieces (two tiles) pass it: HPK_E_INVAL (-1), every dst_off entry 0
    (include/hpk.h), nothing written, and the codec good afterwards."""
    from loona_amd import _lib

    rng = np.random.default_rng(71)
    piece, cap = 1 << 20, 4096
    src = rng.integers(0, 256, piece + 16, dtype=np.uint8)
    starts, lens = np.zeros(n, np.int64), np.full(n, piece, np.int64)
    total = n * piece
    assert (total <= _lib.HPK_MAX_OFFSET) == (n == 4095)
    if n == 4095:
        got, out, intact = _pack_into_view(codec, src, starts, lens, cap, raises=r"hpk_pack_batch failed \(-2\)")
        assert np.array_equal(got, np.arange(n + 1, dtype=np.int64) * piece)
        assert np.array_equal(out, src[:cap])
        assert intact
        return
    got, out, intact = _pack_into_view(codec, src, starts, lens, cap, raises=r"hpk_pack_batch failed \(-1\)")
    assert not got.any(), np.nonzero(got)[0][:5]
    assert (out == CANARY).all() and intact
    codec.check()  # the failing synchronous call cleared the sticky flag
    starts, lens = np.array([7, 100, 40]), np.array([9, 0, 30])
    flat, eoff = gather(src, starts, lens)
    got, out, intact = _pack_into_view(codec, src, starts, lens, int(eoff[-1]))
    assert np.array_equal(got, eoff) and np.array_equal(out, flat) and intact


def test_more_streams_than_slots(codec, request):
    """The packed form and the pack alone on ten streams through one context, which has 8 per-stream slots:
    a 300k-literal batch with long literals on the first stream, then nine 5k-literal batches on the others,
    decode_packed alternating with decode_device + pack, all asynchronous. The ninth stream takes over the
    first one's slot, whose scratch blob the large decode and pack may still be using. One synchronise, then
    every result against the reference decode."""
    from loona_amd import HuffmanCodec, synth

    big = synth.device_config3(codec, n=300_000, seed=505)
    small = [synth.device_config2(codec, n=5_000 + 211 * k, seed=600 + k) for k in range(9)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(10)]
    res = []
    with HuffmanCodec(0, stream="own") as c:
        c.set_decode_kernel(request.node.callspec.params["codec"])
        for k, w in enumerate([big] + small):
            c.set_stream(streams[k])
            if k % 2 == 0:
                pb, po, pl, pst = c.decode_packed(w.enc_blob, w.enc_off)
            else:
                out, oo, pl, pst = c.decode_device(w.enc_blob, w.enc_off)
                pb, po = c.pack(out, oo, pl[: w.n])
            res.append((pb, po, pl, pst))
        torch.cuda.synchronize()
        c.check()
        c.set_stream(torch.cuda.current_stream())
    for k, (w, (pb, po, pl, pst)) in enumerate(zip([big] + small, res)):
        flat, eoff, el, est = expected(w.enc_blob.cpu().numpy(), w.enc_off.cpu().numpy().view(np.uint32))
        assert np.array_equal(po.cpu().numpy().view(np.uint32).astype(np.int64), eoff), f"call {k}: out_off"
        assert np.array_equal(pl[: w.n].cpu().numpy().view(np.uint32), el), f"call {k}: out_len"
        assert np.array_equal(pst[: w.n].cpu().numpy(), est), f"call {k}: status"
        assert np.array_equal(pb.cpu().numpy()[: len(flat)], flat), f"call {k}: bytes"


def test_shard_compact_with_codec(codec):
    """shard.compact(codec=...) equals shard.compact without it, on a region-form and a compacted-form result."""
    from loona_amd import shard, synth

    w = synth.config2(n=30000, seed=12)
    db, do = to_dev(w.enc_blob), to_dev(w.enc_off.view(np.int32))
    for form in ("region", "compacted"):
        fn = codec.decode_device if form == "region" else codec.decode_compact
        out, oo, ol, st = fn(db, do, sync=True)
        total = int(ol[: w.n].to(torch.int64).sum().item())
        a = shard.compact(out, oo, ol, w.n, total)
        b = shard.compact(out, oo, ol, w.n, total, codec=codec)
        torch.cuda.synchronize()
        assert a.shape == b.shape and torch.equal(a, b), form
        assert np.array_equal(b.cpu().numpy(), w.dec_blob[: w.dec_off[-1]]), form
