"""The packed encode on the GPU (hpk_encode_batch_packed, hpk_encoded_len_batch) against the C oracle, bit for
bit: no tolerance. The expected result is always the oracle's: oracle_encode_batch on the same plaintexts,
its valid bytes gathered end to end, the exclusive sum of its lengths (encode_packed_cases.expected).

One checker serves every test: the output view sits `out_shift` bytes into a canary-filled buffer with 4 KiB
guards on both sides, out_off, out_len and status are prefilled with values the call never writes;
afterwards status, out_len and out_off are the oracle's, the bytes below min(total, cap) are the oracle's,
and the canary is intact at and past that point and in both guards. encoded_len_device runs on every case
too and must give the oracle's lengths on its own. The placed cases are proven to reach their cuts in
test_encode_packed_plan.py."""

import numpy as np
import pytest

import encode_cases as ec
import encode_packed_cases as pc
from hpk_util import load, oracle_decode, oracle_encode_batch, pack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CANARY = 0xA5
GUARD = 4096
BAD_N, BAD_J = 20000, 12345


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
    return ec.geometry()


@pytest.fixture(scope="module")
def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def off_dev(a):
    return to_dev(np.asarray(a, np.int64).astype(np.uint32).view(np.int32))


def dev_input(blob, in_shift, in_cap=None):
    """the blob `in_shift` bytes past a 16-byte boundary, as a view of in_cap bytes (default: all of it)"""
    src = np.zeros(in_shift + blob.size + 1, np.uint8)
    src[in_shift : in_shift + blob.size] = blob
    return to_dev(src)[in_shift : in_shift + (blob.size if in_cap is None else in_cap)]


def run_packed(codec, blob, in_off, in_shift, out_shift, cap, sync=True, raises=None, in_cap=None):
    """encode_packed into a view of `cap` bytes -> (view, out_off, out_len, status, guard before, guard after)"""
    n = len(in_off) - 1
    dblob, doff = dev_input(blob, in_shift, in_cap), off_dev(in_off)
    big = torch.full((GUARD + out_shift + cap + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    view = big[GUARD + out_shift : GUARD + out_shift + cap]
    oo = torch.full((n + 1,), -3, dtype=torch.int32, device="cuda")
    ol = torch.full((max(n, 1),), 7, dtype=torch.int32, device="cuda")
    st = torch.full((max(n, 1),), 9, dtype=torch.uint8, device="cuda")
    if raises is None:
        codec.encode_packed(dblob, doff, out_blob=view, out_off=oo, out_len=ol, status=st, sync=sync)
    else:
        with pytest.raises(RuntimeError, match=raises):
            codec.encode_packed(dblob, doff, out_blob=view, out_off=oo, out_len=ol, status=st, sync=True)
    torch.cuda.synchronize()
    g = big.cpu().numpy()
    lead = GUARD + out_shift
    return (g[lead : lead + cap], oo.cpu().numpy().view(np.uint32).astype(np.int64),
            ol[:n].cpu().numpy().view(np.uint32).astype(np.int64), st[:n].cpu().numpy(), g[:lead], g[lead + cap :])


def run_len(codec, blob, in_off, in_shift, sync=True, in_cap=None):
    n = len(in_off) - 1
    ol = torch.full((max(n, 1),), 7, dtype=torch.int32, device="cuda")
    codec.encoded_len_device(dev_input(blob, in_shift, in_cap), off_dev(in_off), out_len=ol, sync=sync)
    torch.cuda.synchronize()
    return ol[:n].cpu().numpy().view(np.uint32).astype(np.int64)


def check(codec, case, what, x=None, cap=None, sync=True, raises=None, lens_too=True):
    """Both calls on a case against the oracle's answer x; cap: the output view's bytes (default: the total)."""
    strs, in_shift, out_shift = case
    x = pc.expected(strs) if x is None else x
    n, total = len(strs), int(x.out_off[-1])
    cap = total if cap is None else cap
    if lens_too:
        got = run_len(codec, x.blob, x.in_off, in_shift)
        bad = np.nonzero(got != x.out_len)[0]
        assert bad.size == 0, f"{what}: encoded_len_device differs at {bad[:10]}: {got[bad[:10]]} for {x.out_len[bad[:10]]}"
    view, oo, ol, st, pre, post = run_packed(codec, x.blob, x.in_off, in_shift, out_shift, cap, sync, raises)
    assert not st.any(), f"{what}: status {st[np.nonzero(st)[0][:10]]} at {np.nonzero(st)[0][:10]}"
    bad = np.nonzero(ol != x.out_len)[0]
    assert bad.size == 0, f"{what}: out_len differs at {bad[:10]}: {ol[bad[:10]]} for {x.out_len[bad[:10]]}"
    assert np.array_equal(oo, x.out_off), f"{what}: out_off is not the exclusive sum of the oracle's lengths"
    k = min(total, cap)
    if not np.array_equal(view[:k], x.flat[:k]):
        first = int(np.nonzero(view[:k] != x.flat[:k])[0][0])
        lit = int(np.searchsorted(x.out_off, first, "right")) - 1
        raise AssertionError(f"{what}: bytes differ first at {first} (literal {lit} of {n}, input bytes "
                             f"{x.in_off[lit]}..{x.in_off[lit + 1]}, output {x.out_off[lit]}..{x.out_off[lit + 1]})")
    assert (view[k:] == CANARY).all(), f"{what}: bytes at or past out_off[n] were written"
    assert (pre == CANARY).all() and (post == CANARY).all(), f"{what}: bytes outside the output view were written"
    return x


# ---- trivial shapes ------------------------------------------------------------------------------

@pytest.mark.parametrize("strs", [[], [b""], [b""] * 5000], ids=["n0", "one_empty", "5000_empty"])
def test_trivial(codec, strs):
    x = check(codec, (strs, 0, 0), "trivial")
    assert x.out_off[-1] == 0
    check(codec, (strs, 3, 5), "trivial, misaligned", x=x, cap=40)


def test_empties_between(codec, geo):
    check(codec, pc.empties_between(geo), "empties between")


# ---- reference plaintexts, every byte value --------------------------------------------------------

def test_reference_plaintexts(codec):
    """the plaintexts of the KATs and of the RFC 7541 App. C literals (their oracle decode)"""
    vecs = load("kat.json") + load("rfc7541_blocks.json")["huffman_literals"]
    strs, wires = [], []
    for v in vecs:
        st, plain = oracle_decode(bytes.fromhex(v["in"]))
        assert st == v.get("status", 0) and (st != 0 or plain == bytes.fromhex(v["out"]))
        strs.append(plain)  # (an error vector: the bytes decoded before its error)
        wires.append(bytes.fromhex(v["in"]) if st == 0 else None)
    assert sum(w is not None for w in wires) >= 20
    x = check(codec, (strs, 0, 0), "reference plaintexts")
    for i, w in enumerate(wires):  # and a valid vector's encoding is the vector itself
        assert w is None or x.flat[x.out_off[i] : x.out_off[i + 1]].tobytes() == w


def test_every_byte_value(codec):
    from loona_amd import _lib

    strs = [bytes((b,)) for b in range(256)] + [bytes((b,)) * 8 for b in range(256)]
    x = check(codec, (strs, 0, 0), "every byte value")
    L = _lib.lib()
    want = np.array([L.hpk_huffman_encoded_len(s, len(s)) for s in strs], np.int64)
    assert np.array_equal(run_len(codec, x.blob, x.in_off, 0), want)


# ---- misalignment ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def text3000():
    strs = pc.text_batch(3000, 120, 14000)[0]
    return strs, pc.expected(strs)


@pytest.mark.parametrize("in_shift", [0, 1, 15])
@pytest.mark.parametrize("out_shift", [0, 1, 15])
def test_misalignment(codec, text3000, in_shift, out_shift):
    strs, x = text3000
    check(codec, (strs, in_shift, out_shift), f"misaligned in{in_shift} out{out_shift}", x=x)


# ---- input cuts -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("plus", [0, 1])
@pytest.mark.parametrize("shift", [0, 5])
def test_in_cut(codec, geo, plus, shift):
    check(codec, pc.in_cut(geo, plus, shift), f"in cut T+{plus} in{shift}")


@pytest.mark.parametrize("e", [1, 33])
def test_empties_on_cut(codec, geo, e):
    check(codec, pc.empties_on_cut(geo, e), f"{e} empties on the cut")


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("size", ["T", "T_plus1", "3T_plus5"])
def test_lone_literal(codec, geo, size, shift):
    nbytes = dict(zip(("T", "T_plus1", "3T_plus5"), pc.lone_sizes(geo)))[size]
    check(codec, pc.lone(geo, nbytes, shift), f"lone literal of {nbytes} bytes, in{shift}")


def test_lone_literal_short_capacity(codec, geo):
    """a lone literal of 3 T + 5 bytes (the one-lane encode path) into half its encoding: the path's own clip"""
    case = pc.lone(geo, 3 * geo.T + 5, 1)
    x = pc.expected(case[0])
    total = int(x.out_off[-1])
    for cap in (total // 2, 1, total - 1):
        check(codec, (case[0], 1, 7), f"lone literal, cap {cap}", x=x, cap=cap, raises=r"\(-2\)", lens_too=False)
        check(codec, (case[0], 1, 7), f"lone literal, cap {cap}, async", x=x, cap=cap, sync=False, lens_too=False)
    codec.check()


def test_one_mib_literal(codec, geo):
    check(codec, pc.lone(geo, 1 << 20, 3), "one 1 MiB literal")


# ---- count cut, output cut, many workgroups ------------------------------------------------------------------

@pytest.mark.parametrize("one_byte", [False, True], ids=["empty", "one_byte"])
def test_count_cut(codec, geo, cus, one_byte):
    check(codec, pc.count_cut(geo, cus, one_byte), "count cut")


@pytest.mark.parametrize("kind", ["thirty", "five", "alternate"])
def test_out_cut_exact_regions(codec, geo, kind):
    check(codec, pc.out_cut(geo, kind), f"output cut, {kind}")


def test_multi_workgroup(codec):
    check(codec, pc.multi_wg(), "20 000 text literals", x=pc.multi_wg_expected())


# ---- capacity -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cap_batch():
    strs = pc.text_batch(4000, 100, 15000)[0]
    return strs, pc.expected(strs)


def cap_values(x):
    total = int(x.out_off[-1])
    mid = int(np.nonzero(x.out_len > 2)[0][len(x.out_len) // 4])
    return {"total": total, "total_minus1": total - 1, "mid_literal": int(x.out_off[mid]) + 1,
            "literal_boundary": int(x.out_off[len(x.out_len) // 2]), "zero": 0}


@pytest.mark.parametrize("which", ["total", "total_minus1", "mid_literal", "literal_boundary", "zero"])
@pytest.mark.parametrize("out_shift", [0, 9])
def test_capacity(codec, cap_batch, which, out_shift):
    strs, x = cap_batch
    cap = cap_values(x)[which]
    total = int(x.out_off[-1])
    assert 0 <= cap <= total and (cap == total) == (which == "total")
    if which == "mid_literal":
        assert cap not in set(x.out_off.tolist())
    if which == "literal_boundary":
        assert 0 < cap < total and cap in set(x.out_off.tolist())
    short = cap < total
    # synchronous: -2 (HPK_E_NOSPACE) when short; asynchronous: returns; everything else complete either way
    check(codec, (strs, 0, out_shift), f"cap {which} sync", x=x, cap=cap, raises=r"\(-2\)" if short else None,
          lens_too=False)
    check(codec, (strs, 0, out_shift), f"cap {which} async", x=x, cap=cap, sync=False, lens_too=False)
    codec.check()  # no sticky error was left


# ---- bad offsets -----------------------------------------------------------------------------------------------------

def check_bad(codec, blob, in_off, bad, what, in_cap=None, cap=None):
    """A batch with bad offsets at the literals `bad`: -1 from both calls, status 5 and out_len 0 there, out_off
    the exclusive sum of the returned out_len, and every status-0 literal holds the oracle's encoding of its
    own bytes (the call may void other literals)."""
    n = len(in_off) - 1
    icap = blob.size if in_cap is None else in_cap
    good = np.nonzero((in_off[:-1] <= in_off[1:]) & (in_off[1:] <= icap))[0]
    assert not set(good.tolist()) & set(bad) and len(good) + len(bad) == n
    gblob, goff = pack([blob[in_off[i] : in_off[i + 1]].tobytes() for i in good])
    ob, oo_, gl, gst = oracle_encode_batch(gblob, goff)
    assert not gst.any()
    want_len = np.zeros(n, np.int64)
    want_len[good] = gl
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        run_len(codec, blob, in_off, 0, in_cap=in_cap)
    lens = run_len(codec, blob, in_off, 0, sync=False, in_cap=in_cap)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        codec.check()
    assert np.array_equal(lens, want_len), f"{what}: encoded_len_device counts 0 for exactly the bad literals"
    total = int(want_len.sum())
    cap = total if cap is None else cap
    view, oo, ol, st, pre, post = run_packed(codec, blob, in_off, 0, 0, cap, raises=r"\(-1\)", in_cap=in_cap)
    assert set(np.unique(st).tolist()) <= {0, 5}
    assert (st[list(bad)] == 5).all() and not ol[st == 5].any(), what
    ok = np.nonzero(st == 0)[0]
    assert np.array_equal(ol[ok], want_len[ok]), f"{what}: out_len of the literals that were not voided"
    eoff = np.zeros(n + 1, np.int64)
    np.cumsum(ol, out=eoff[1:])
    assert np.array_equal(oo, eoff), f"{what}: out_off is not the exclusive sum of out_len"
    # the bytes of the status-0 literals, as far as the capacity goes
    gpos = np.full(n, -1, np.int64)
    gpos[good] = np.arange(len(good))
    k = min(int(eoff[-1]), cap)
    want = np.full(k, -1, np.int64)
    for i in ok:
        a, b = int(eoff[i]), min(int(eoff[i + 1]), k)
        if a < b:
            s = int(oo_[gpos[i]])
            want[a:b] = ob[s : s + b - a]
    assert (want >= 0).all() and np.array_equal(view[:k], want.astype(np.uint8)), f"{what}: bytes of the good literals"
    assert (view[k:] == CANARY).all() and (pre == CANARY).all() and (post == CANARY).all(), what
    return total


def test_bad_offsets_decreasing(codec):
    strs = pc.text_batch(BAD_N, 60, 16000)[0]
    blob, off = pack(strs)
    off = off.astype(np.int64)
    assert off[BAD_J + 1] - off[BAD_J] > 5
    off[BAD_J + 1] = off[BAD_J] - 3  # literal BAD_J decreases; BAD_J + 1 starts 3 bytes earlier and is good
    total = check_bad(codec, blob, off, [BAD_J], "decreasing offsets")
    check_bad(codec, blob, off, [BAD_J], "decreasing offsets, short capacity", cap=total // 2)


def test_bad_offsets_past_in_cap(codec, geo):
    """in_off passes in_cap in the second tile of a batch of at most P literals (one workgroup)"""
    rng = np.random.default_rng(17000)
    lens = [geo.T // 8] * 12 + [50] * 20
    assert len(lens) <= geo.P
    blob, off = pack([ec._text(rng, k) for k in lens])
    off = off.astype(np.int64)
    plan = ec.tile_plan(off, pc.expected([blob[off[i] : off[i + 1]].tobytes() for i in range(len(lens))]).out_off, 0, 0, geo)
    first_bad = 10
    assert plan[0] == (0, 8, "input") and plan[1][0] == 8 and plan[1][0] < first_bad < plan[1][0] + plan[1][1]
    in_cap = int(off[first_bad + 1]) - 1  # literal 10 and every literal after it pass the capacity
    bad = list(range(first_bad, len(lens)))
    total = check_bad(codec, blob, off, bad, "offsets past in_cap", in_cap=in_cap)
    check_bad(codec, blob, off, bad, "offsets past in_cap, short capacity", in_cap=in_cap, cap=total - 7)


# ---- round trip -----------------------------------------------------------------------------------------------------

def test_round_trip(codec):
    strs = pc.multi_wg()[0]
    x = pc.multi_wg_expected()
    eb, eo, el, est = codec.encode_packed(to_dev(x.blob), off_dev(x.in_off), sync=True)
    assert eb.numel() == int(x.out_off[-1])  # (the blob sized by one host read of the lengths' total)
    db, do, dl, dst = codec.decode_packed(eb, eo, sync=True)  # out_off feeds straight in as in_off
    assert not dst.any().item()
    assert np.array_equal(do.cpu().numpy().view(np.uint32).astype(np.int64), x.in_off)
    assert np.array_equal(db.cpu().numpy(), x.blob)
    eb2 = codec.encode_packed(to_dev(x.blob), off_dev(x.in_off))[0]  # asynchronous: the bound-sized blob
    torch.cuda.synchronize()
    assert eb2.numel() == (30 * x.blob.size + 7) // 8 and np.array_equal(eb2[: eb.numel()].cpu().numpy(), x.flat)


def test_own_stream_allocates_from_the_lengths():
    """encode_packed(sync=True) with no out_blob on a codec that runs on its own stream, not torch's current
    one: the blob is sized by a host read of the lengths' total, which must wait for the length pass."""
    from loona_amd import HuffmanCodec

    x = pc.multi_wg_expected()
    dblob, doff = to_dev(x.blob), off_dev(x.in_off)
    torch.cuda.synchronize()  # (the inputs were made on torch's stream)
    with HuffmanCodec(0, stream="own") as c:
        for _ in range(3):
            eb, eo, el, est = c.encode_packed(dblob, doff, sync=True)
            assert eb.numel() == int(x.out_off[-1])
            assert np.array_equal(eo.cpu().numpy().view(np.uint32).astype(np.int64), x.out_off)
            assert np.array_equal(el.cpu().numpy().view(np.uint32).astype(np.int64), x.out_len)
            assert not est.any().item() and np.array_equal(eb.cpu().numpy(), x.flat)


# ---- a total past HPK_MAX_OFFSET ----------------------------------------------------------------------------------------

def test_total_past_max_offset(codec):
    """1 000 literals over 1.15e9 bytes of value 10 (a 30-bit code): 4.3e9 encoded bytes. Every literal is void
    and every offset 0; the capacity is 0 and no byte is written. (One run: the only case above a few MB.)"""
    nbytes, n = 1_150_000_000, 1000
    try:
        blob = torch.full((nbytes,), 10, dtype=torch.uint8, device="cuda")
    except RuntimeError as e:  # (out of memory)
        pytest.skip(f"cannot allocate the {nbytes}-byte input: {e}")
    off = (np.arange(n + 1, dtype=np.int64) * (nbytes // n)).astype(np.uint32).view(np.int32)
    assert 30 * int(off[-1]) // 8 > 0xFFFFFFDF
    doff = to_dev(off)
    oo = torch.full((n + 1,), -3, dtype=torch.int32, device="cuda")
    ol = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    big = torch.full((2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    lens = codec.encoded_len_device(blob, doff, sync=True)  # the lengths alone are fine: each fits
    assert (lens[:n].cpu().numpy().astype(np.int64) == (30 * (nbytes // n) + 7) // 8).all()
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        codec.encode_packed(blob, doff, out_blob=big[GUARD:GUARD], out_off=oo, out_len=ol, status=st, sync=True)
    torch.cuda.synchronize()
    assert not oo.cpu().numpy().any() and not ol.cpu().numpy().any() and (st.cpu().numpy() == 5).all()
    assert (big.cpu().numpy() == CANARY).all()
