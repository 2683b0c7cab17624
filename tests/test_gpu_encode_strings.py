"""The packed string-literal encode on the GPU (hpk_encode_strings_packed, hpk_string_len_batch), byte for
byte: no tolerance. The expected result is encode_strings_cases.expected(): the C oracle's Huffman payloads and
hpack_ref.encode_integer's prefixes under the rule of hpack_ref.Encoder._string, never the code under test.

One checker serves every case, in the shape of test_gpu_encode_packed.check: the output view sits `out_shift`
bytes into a canary-filled buffer with 4 KiB guards on both sides, out_off, out_len and status are prefilled
with values the call never writes; afterwards status, out_len and out_off are the expected ones, the bytes below
min(total, cap) are the expected ones, and the canary is intact at and past that point and in both guards.
string_len_device runs on every case too. The placed cases are proven to reach their cuts in
test_encode_strings_plan.py."""

import numpy as np
import pytest

import encode_packed_cases as pc
import encode_strings_cases as sc
from hpk_util import hpack_ref, pack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CANARY = 0xA5
GUARD = 4096


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
    return sc.geometry()


@pytest.fixture(scope="module")
def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def off_dev(a):
    return to_dev(np.asarray(a, np.int64).astype(np.uint32).view(np.int32))


def dev_input(blob, in_shift, in_cap=None):
    src = np.zeros(in_shift + blob.size + 1, np.uint8)
    src[in_shift : in_shift + blob.size] = blob
    return to_dev(src)[in_shift : in_shift + (blob.size if in_cap is None else in_cap)]


def pol_dev(policy):
    return None if policy is None else to_dev(np.asarray(policy, np.uint8))


def run_strings(codec, blob, in_off, policy, in_shift, out_shift, cap, sync=True, raises=None, in_cap=None):
    """encode_strings into a view of `cap` bytes -> (view, out_off, out_len, status, guard before, guard after)"""
    n = len(in_off) - 1
    dblob, doff, dpol = dev_input(blob, in_shift, in_cap), off_dev(in_off), pol_dev(policy)
    big = torch.full((GUARD + out_shift + cap + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    view = big[GUARD + out_shift : GUARD + out_shift + cap]
    oo = torch.full((n + 1,), -3, dtype=torch.int32, device="cuda")
    ol = torch.full((max(n, 1),), 7, dtype=torch.int32, device="cuda")
    st = torch.full((max(n, 1),), 9, dtype=torch.uint8, device="cuda")
    if raises is None:
        codec.encode_strings(dblob, doff, dpol, out_blob=view, out_off=oo, out_len=ol, status=st, sync=sync)
    else:
        with pytest.raises(RuntimeError, match=raises):
            codec.encode_strings(dblob, doff, dpol, out_blob=view, out_off=oo, out_len=ol, status=st, sync=True)
    torch.cuda.synchronize()
    g = big.cpu().numpy()
    lead = GUARD + out_shift
    return (g[lead : lead + cap], oo.cpu().numpy().view(np.uint32).astype(np.int64),
            ol[:n].cpu().numpy().view(np.uint32).astype(np.int64), st[:n].cpu().numpy(), g[:lead], g[lead + cap :])


def run_len(codec, blob, in_off, policy, in_shift, sync=True, in_cap=None):
    n = len(in_off) - 1
    ol = torch.full((max(n, 1),), 7, dtype=torch.int32, device="cuda")
    codec.string_len_device(dev_input(blob, in_shift, in_cap), off_dev(in_off), pol_dev(policy), out_len=ol, sync=sync)
    torch.cuda.synchronize()
    return ol[:n].cpu().numpy().view(np.uint32).astype(np.int64)


def check(codec, case, what, x=None, cap=None, sync=True, raises=None, lens_too=True):
    """Both calls on a case against the expected answer x; cap: the output view's bytes (default: the total)."""
    strs, policy, in_shift, out_shift = case
    x = sc.expected(strs, policy) if x is None else x
    n, total = len(strs), int(x.out_off[-1])
    cap = total if cap is None else cap
    if lens_too:
        got = run_len(codec, x.blob, x.in_off, policy, in_shift)
        bad = np.nonzero(got != x.out_len)[0]
        assert bad.size == 0, f"{what}: string_len_device differs at {bad[:10]}: {got[bad[:10]]} for {x.out_len[bad[:10]]}"
    view, oo, ol, st, pre, post = run_strings(codec, x.blob, x.in_off, policy, in_shift, out_shift, cap, sync, raises)
    assert not st.any(), f"{what}: status {st[np.nonzero(st)[0][:10]]} at {np.nonzero(st)[0][:10]}"
    bad = np.nonzero(ol != x.out_len)[0]
    assert bad.size == 0, f"{what}: out_len differs at {bad[:10]}: {ol[bad[:10]]} for {x.out_len[bad[:10]]}"
    assert np.array_equal(oo, x.out_off), f"{what}: out_off is not the exclusive sum of the expected lengths"
    k = min(total, cap)
    if not np.array_equal(view[:k], x.flat[:k]):
        first = int(np.nonzero(view[:k] != x.flat[:k])[0][0])
        lit = int(np.searchsorted(x.out_off, first, "right")) - 1
        raise AssertionError(f"{what}: bytes differ first at {first} (literal {lit} of {n}, policy {x.policy[lit]}, "
                             f"input bytes {x.in_off[lit]}..{x.in_off[lit + 1]}, output {x.out_off[lit]}.."
                             f"{x.out_off[lit + 1]}): {view[first]:#x} for {x.flat[first]:#x}")
    assert (view[k:] == CANARY).all(), f"{what}: bytes at or past out_off[n] were written"
    assert (pre == CANARY).all() and (post == CANARY).all(), f"{what}: bytes outside the output view were written"
    return x


# ---- trivial shapes ------------------------------------------------------------------------------

def test_n0(codec):
    x = check(codec, ([], None, 0, 0), "n = 0")
    assert x.out_off.tolist() == [0]
    check(codec, ([], None, 3, 5), "n = 0, misaligned", x=x, cap=40)


@pytest.mark.parametrize("pol,want", [(sc.AUTO, "00"), (sc.RAW, "00"), (sc.HUFFMAN, "80"), (sc.VERBATIM, "")])
def test_one_empty(codec, pol, want):
    x = check(codec, ([b""], sc.policies(1, pol), 0, 0), "one empty literal")
    assert x.flat.tobytes().hex() == want
    check(codec, ([b""], sc.policies(1, pol), 3, 5), "one empty literal, misaligned", x=x, cap=40)


@pytest.mark.parametrize("pol", [None, sc.VERBATIM], ids=["auto", "verbatim"])
def test_5000_empties(codec, pol):
    policy = None if pol is None else sc.policies(5000, pol)
    x = check(codec, ([b""] * 5000, policy, 0, 0), "5000 empties")
    assert x.out_off[-1] == (5000 if pol is None else 0)
    check(codec, ([b""] * 5000, policy, 3, 5), "5000 empties, misaligned", x=x, cap=int(x.out_off[-1]) + 40)


# ---- RFC 7541 C.4 ------------------------------------------------------------------------------------

def test_rfc_c4(codec):
    strs = [b"www.example.com", b"no-cache", b"custom-key", b"custom-value"]
    x = check(codec, (strs, None, 0, 0), "RFC 7541 C.4 literals")
    want = ["8cf1e3c2e5f23a6ba0ab90f4ff", "86a8eb10649cbf", "8825a849e95ba97d7f", "8925a849e95bb8e8b4bf"]
    assert [x.flat[x.out_off[i] : x.out_off[i + 1]].tobytes().hex() for i in range(4)] == want
    x = check(codec, (strs, sc.policies(4, sc.RAW), 0, 0), "RFC 7541 C.4 literals, raw")
    assert x.flat[: x.out_off[1]].tobytes() == b"\x0f" + strs[0]


# ---- the decision edge, the prefix edges ------------------------------------------------------------

def test_decision_edge(codec):
    strs, huff = sc.decision_edge()
    x = check(codec, (strs, None, 0, 0), "decision edge")
    assert np.array_equal(x.huff, huff)
    x = check(codec, ([bytes((b,)) for b in range(256)], None, 0, 0), "every byte value alone")
    assert not x.huff.any()
    x = check(codec, ([bytes((a, b)) for a in b"012aceiost" for b in b"012aceiost"], None, 1, 1), "two 5-bit codes")
    assert not x.huff.any()


def test_prefix_edges(codec):
    strs, pol, pay, huff = sc.prefix_edges_small()
    check(codec, (strs, pol, 0, 0), "prefix edges")
    check(codec, (strs, pol, 5, 11), "prefix edges, misaligned")


@pytest.mark.parametrize("p", sc.PREFIX_EDGES_RAW_ONLY)
def test_prefix_edges_4_and_5_octets(codec, p):
    rng = np.random.default_rng(p)
    strs = [b"ab", rng.integers(0, 256, p, dtype=np.uint8).tobytes(), b"cd"]
    x = check(codec, (strs, sc.policies(3, sc.RAW), 0, 3), f"raw payload of {p} bytes")
    assert x.plen[1] == (4 if p == 2097278 else 5)


# ---- misalignment ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed3000():
    strs, pol = sc.mixed_batch(3000, 300, 25000)
    return strs, pol, sc.expected(strs, pol)


@pytest.mark.parametrize("in_shift", [0, 1, 15])
@pytest.mark.parametrize("out_shift", [0, 1, 15])
def test_misalignment(codec, mixed3000, in_shift, out_shift):
    strs, pol, x = mixed3000
    check(codec, (strs, pol, in_shift, out_shift), f"misaligned in{in_shift} out{out_shift}", x=x,
          lens_too=out_shift == 0)


def test_prefix_straddles_every_chunk_position(codec):
    strs, pol = sc.prefix_straddle()
    x = sc.expected(strs, pol)
    at = set()
    for sh in range(16):
        check(codec, (strs, pol, 0, sh), f"prefix straddle, out{sh}", x=x, lens_too=sh == 0)
        at |= {(int(o) + sh) % 16 for o in x.out_off[:-1]}
    assert at == set(range(16))


# ---- placed cuts --------------------------------------------------------------------------------------

@pytest.mark.parametrize("plus", [0, 1])
@pytest.mark.parametrize("shift", [0, 5])
def test_in_cut(codec, geo, plus, shift):
    strs, sh, _ = pc.in_cut(geo, plus, shift)
    check(codec, (strs, None, sh, 0), f"in cut T+{plus} in{shift}")
    check(codec, (strs, sc.policies(len(strs), sc.RAW), sh, 0), f"in cut T+{plus} in{shift}, raw")


@pytest.mark.parametrize("e", [1, 33])
def test_empties_on_cut(codec, geo, e):
    check(codec, (pc.empties_on_cut(geo, e)[0], None, 0, 0), f"{e} empties on the cut")


@pytest.mark.parametrize("one_byte", [False, True], ids=["empty", "one_byte"])
def test_count_cut(codec, geo, cus, one_byte):
    check(codec, (pc.count_cut(geo, cus, one_byte)[0], None, 0, 0), "count cut")


@pytest.mark.parametrize("kind", ["thirty", "five", "alternate"])
def test_out_cut(codec, geo, kind):
    strs = pc.out_cut(geo, kind)[0]
    check(codec, (strs, sc.policies(len(strs), sc.HUFFMAN), 0, 0), f"output cut, {kind}, Huffman")
    check(codec, (strs, None, 0, 0), f"output cut, {kind}, auto")


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("size", ["T", "T_plus1", "3T_plus5"])
def test_lone_literal(codec, geo, size, shift):
    nbytes = dict(zip(("T", "T_plus1", "3T_plus5"), pc.lone_sizes(geo)))[size]
    strs = sc.lone(nbytes, shift)
    for pol in (sc.RAW, sc.AUTO, sc.VERBATIM):
        check(codec, (strs, sc.policies(1, pol), shift, shift), f"lone literal of {nbytes} bytes, policy {pol}")


# ---- many workgroups ------------------------------------------------------------------------------------

def test_multi_workgroup_text(codec):
    check(codec, (pc.multi_wg()[0], None, 0, 0), "20 000 text literals", x=sc.multi_wg_expected())


def test_multi_workgroup_uniform(codec):
    check(codec, (sc.uniform_batch(20000, 300, 24000), None, 0, 0), "20 000 uniform-byte literals")


# ---- capacity -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cap_batch():
    strs, pol = sc.mixed_batch(4000, 400, 26000)
    pol[pol == sc.VERBATIM] = sc.RAW
    return strs, pol, sc.expected(strs, pol)


def cap_values(x):
    total = int(x.out_off[-1])
    n = len(x.out_len)
    two = int(np.nonzero(x.plen >= 2)[0][n // 8])  # between the two prefix octets of one literal
    mid = int(np.nonzero(x.out_len > 8)[0][n // 8])
    return {"total": total, "total_minus1": total - 1, "in_prefix": int(x.out_off[two]) + 1,
            "mid_payload": int(x.out_off[mid]) + int(x.plen[mid]) + 2, "literal_boundary": int(x.out_off[n // 2]),
            "zero": 0}


@pytest.mark.parametrize("which", ["total", "total_minus1", "in_prefix", "mid_payload", "literal_boundary", "zero"])
@pytest.mark.parametrize("out_shift", [0, 9])
def test_capacity(codec, cap_batch, which, out_shift):
    strs, pol, x = cap_batch
    cap = cap_values(x)[which]
    total = int(x.out_off[-1])
    assert 0 <= cap <= total and (cap == total) == (which == "total")
    if which in ("in_prefix", "mid_payload"):
        assert cap not in set(x.out_off.tolist())
    if which == "literal_boundary":
        assert 0 < cap < total and cap in set(x.out_off.tolist())
    short = cap < total
    check(codec, (strs, pol, 0, out_shift), f"cap {which} sync", x=x, cap=cap, raises=r"\(-2\)" if short else None,
          lens_too=False)
    check(codec, (strs, pol, 0, out_shift), f"cap {which} async", x=x, cap=cap, sync=False, lens_too=False)
    codec.check()  # no sticky error was left


def test_lone_literal_short_capacity(codec, geo):
    """the large-literal paths' own clips: a raw and a Huffman literal of 3 T + 5 bytes into part of the room"""
    strs = sc.lone(3 * geo.T + 5, 1)
    for pol in (sc.RAW, sc.AUTO):
        x = sc.expected(strs, sc.policies(1, pol))
        total = int(x.out_off[-1])
        for cap in (total // 2, 1, 2, total - 1):
            check(codec, (strs, sc.policies(1, pol), 1, 7), f"lone literal, policy {pol}, cap {cap}", x=x, cap=cap,
                  raises=r"\(-2\)", lens_too=False)
    codec.check()


# ---- bad input -----------------------------------------------------------------------------------------------

def check_bad(codec, blob, in_off, policy, bad, what, in_cap=None, cap=None):
    """A batch whose literals `bad` have bad offsets or a bad policy: -1 from both calls, status 5 and out_len 0
    there, out_off the exclusive sum of the returned out_len, and every status-0 literal holds the expected
    representation of its own bytes (the contract lets the call void other literals too)."""
    n = len(in_off) - 1
    pol = np.zeros(n, np.uint8) if policy is None else np.asarray(policy, np.uint8)
    icap = blob.size if in_cap is None else in_cap
    good = np.nonzero((in_off[:-1] <= in_off[1:]) & (in_off[1:] <= icap) & (pol <= 3))[0]
    assert not set(good.tolist()) & set(bad) and len(good) + len(bad) == n
    g = sc.expected([blob[in_off[i] : in_off[i + 1]].tobytes() for i in good], pol[good])
    want_len = np.zeros(n, np.int64)
    want_len[good] = g.out_len
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        run_len(codec, blob, in_off, policy, 0, in_cap=in_cap)
    lens = run_len(codec, blob, in_off, policy, 0, sync=False, in_cap=in_cap)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        codec.check()
    assert np.array_equal(lens, want_len), f"{what}: string_len_device counts 0 for exactly the bad literals"
    total = int(want_len.sum())
    cap = total if cap is None else cap
    view, oo, ol, st, pre, post = run_strings(codec, blob, in_off, policy, 0, 0, cap, raises=r"\(-1\)", in_cap=in_cap)
    assert set(np.unique(st).tolist()) <= {0, 5}
    assert (st[list(bad)] == 5).all() and not ol[st == 5].any(), what
    ok = np.nonzero(st == 0)[0]
    assert np.array_equal(ol[ok], want_len[ok]), f"{what}: out_len of the literals that were not voided"
    eoff = np.zeros(n + 1, np.int64)
    np.cumsum(ol, out=eoff[1:])
    assert np.array_equal(oo, eoff), f"{what}: out_off is not the exclusive sum of out_len"
    gpos = np.full(n, -1, np.int64)
    gpos[good] = np.arange(len(good))
    k = min(int(eoff[-1]), cap)
    want = np.full(k, -1, np.int64)
    for i in ok:
        a, b = int(eoff[i]), min(int(eoff[i + 1]), k)
        if a < b:
            s = int(g.out_off[gpos[i]])
            want[a:b] = g.flat[s : s + b - a]
    assert (want >= 0).all() and np.array_equal(view[:k], want.astype(np.uint8)), f"{what}: bytes of the good literals"
    assert (view[k:] == CANARY).all() and (pre == CANARY).all() and (post == CANARY).all(), what
    return total


BAD_N, BAD_J = 6000, 3456


def test_bad_offsets_decreasing(codec):
    strs, pol = sc.mixed_batch(BAD_N, 120, 27000)
    strs[BAD_J] = b"0123456789"
    blob, off = pack(strs)
    off = off.astype(np.int64)
    off[BAD_J + 1] = off[BAD_J] - 3  # literal BAD_J decreases; BAD_J + 1 starts 3 bytes earlier and is good
    total = check_bad(codec, blob, off, pol, [BAD_J], "decreasing offsets")
    check_bad(codec, blob, off, pol, [BAD_J], "decreasing offsets, short capacity", cap=total // 2)


def test_bad_offsets_past_in_cap(codec, geo):
    """in_off passes in_cap in the second tile of a batch of at most P literals (one workgroup)"""
    import encode_cases as ec

    rng = np.random.default_rng(17000)
    lens = [geo.T // 8] * 12 + [50] * 20
    assert len(lens) <= geo.P
    strs = [ec._text(rng, k) for k in lens]
    blob, off = pack(strs)
    off = off.astype(np.int64)
    plan = ec.tile_plan(off, sc.expected(strs).out_off, 0, 0, geo)
    first_bad = 10
    assert plan[0] == (0, 8, "input") and plan[1][0] == 8 and plan[1][0] < first_bad < plan[1][0] + plan[1][1]
    in_cap = int(off[first_bad + 1]) - 1  # literal 10 and every literal after it pass the capacity
    bad = list(range(first_bad, len(lens)))
    total = check_bad(codec, blob, off, None, bad, "offsets past in_cap", in_cap=in_cap)
    check_bad(codec, blob, off, None, bad, "offsets past in_cap, short capacity", in_cap=in_cap, cap=total - 7)


def test_bad_policy(codec):
    strs, pol = sc.mixed_batch(2000, 120, 28000)
    blob, off = pack(strs)
    pol[777] = 4
    pol[1500] = 255
    check_bad(codec, blob, off.astype(np.int64), pol, [777, 1500], "a policy byte of 4")


# ---- a total past HPK_MAX_OFFSET ----------------------------------------------------------------------------------

def test_total_past_max_offset(codec):
    """1 000 literals over 1.15e9 bytes of value 10 (a 30-bit code) under HUFFMAN: 4.3e9 bytes. Every literal is
    void and every offset 0; the capacity is 0 and no byte is written. (One run: the only case above a few MB.)"""
    nbytes, n = 1_150_000_000, 1000
    try:
        blob = torch.full((nbytes,), 10, dtype=torch.uint8, device="cuda")
    except RuntimeError as e:  # (out of memory)
        pytest.skip(f"cannot allocate the {nbytes}-byte input: {e}")
    off = (np.arange(n + 1, dtype=np.int64) * (nbytes // n)).astype(np.uint32).view(np.int32)
    assert 30 * int(off[-1]) // 8 > 0xFFFFFFDF
    doff = to_dev(off)
    dpol = to_dev(sc.policies(n, sc.HUFFMAN))
    oo = torch.full((n + 1,), -3, dtype=torch.int32, device="cuda")
    ol = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    big = torch.full((2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    lens = codec.string_len_device(blob, doff, dpol, sync=True)  # the lengths alone are fine: each fits
    payload = (30 * (nbytes // n) + 7) // 8
    assert (lens[:n].cpu().numpy().astype(np.int64) == payload + len(hpack_ref.encode_integer(payload, 7))).all()
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        codec.encode_strings(blob, doff, dpol, out_blob=big[GUARD:GUARD], out_off=oo, out_len=ol, status=st, sync=True)
    torch.cuda.synchronize()
    assert not oo.cpu().numpy().any() and not ol.cpu().numpy().any() and (st.cpu().numpy() == 5).all()
    assert (big.cpu().numpy() == CANARY).all()


# ---- allocation rules -------------------------------------------------------------------------------------------

def test_allocates_from_the_lengths(codec, mixed3000):
    strs, pol, x = mixed3000
    eb, eo, el, est = codec.encode_strings(to_dev(x.blob), off_dev(x.in_off), to_dev(pol), sync=True)
    assert eb.numel() == int(x.out_off[-1]) and np.array_equal(eb.cpu().numpy(), x.flat)
    eb2 = codec.encode_strings(to_dev(x.blob), off_dev(x.in_off), to_dev(pol))[0]  # asynchronous: the bound
    torch.cuda.synchronize()
    assert eb2.numel() >= eb.numel() and np.array_equal(eb2[: eb.numel()].cpu().numpy(), x.flat)


# ---- the host form ------------------------------------------------------------------------------------------------

def test_host_form(codec, mixed3000):
    strs, pol, x = mixed3000
    ob, oo, ol, st = codec.encode_strings_host(x.blob, x.in_off, pol)
    assert not st.any() and np.array_equal(ol.astype(np.int64), x.out_len)
    assert np.array_equal(oo.astype(np.int64), x.out_off) and np.array_equal(ob, x.flat)
    a = sc.expected(strs)  # no policy array: all AUTO
    ob, oo, ol, st = codec.encode_strings_host(a.blob, a.in_off)
    assert np.array_equal(oo.astype(np.int64), a.out_off) and np.array_equal(ob, a.flat)
    ob, oo, ol, st = codec.encode_strings_host(np.zeros(0, np.uint8), np.zeros(1, np.uint32))
    assert ob.size == 0 and oo.tolist() == [0]


def host_call(codec, blob, off, pol, cap):
    """the host form into prefilled arrays -> (out_blob, out_off, out_len, status, the error or None)"""
    n = len(off) - 1
    out = np.full(max(cap, 1), CANARY, np.uint8)[:cap]
    oo, ol = np.full(n + 1, 0xFFFFFFFD, np.uint32), np.full(max(n, 1), 7, np.uint32)
    st = np.full(max(n, 1), 9, np.uint8)
    err = None
    try:
        codec._strings_call(np.ascontiguousarray(blob, np.uint8), np.ascontiguousarray(off, np.uint32), pol, out, oo, ol,
                            st, False, True)
    except RuntimeError as e:
        err = str(e)
    return out, oo, ol, st, err


def test_host_form_refuses_bad_input(codec, mixed3000):
    strs, pol, x = mixed3000
    total = int(x.out_off[-1])
    off = x.in_off.copy()
    off[100] = off[99] - 1
    badpol = pol.copy()
    badpol[2999] = 4
    past = x.in_off.copy()
    past[-1] += 1
    for what, o, p in (("decreasing offsets", off, pol), ("a policy byte of 4", x.in_off, badpol),
                       ("offsets past in_cap", past, pol)):
        out, oo, ol, st, err = host_call(codec, x.blob, o, p, total)
        assert err is not None and "(-1)" in err, what
        assert (out == CANARY).all() and (oo == 0xFFFFFFFD).all() and (ol == 7).all() and (st == 9).all(), what
    codec.check()


def test_host_form_nospace(codec, mixed3000):
    strs, pol, x = mixed3000
    total = int(x.out_off[-1])
    cap = total // 2 + 1
    out, oo, ol, st, err = host_call(codec, x.blob, x.in_off, pol, cap)
    assert err is not None and "(-2)" in err
    assert np.array_equal(oo.astype(np.int64), x.out_off) and np.array_equal(ol.astype(np.int64), x.out_len)
    assert not st.any() and np.array_equal(out, x.flat[:cap])
    out, oo, ol, st, err = host_call(codec, x.blob, x.in_off, pol, total)
    assert err is None and np.array_equal(out, x.flat)


# ---- header blocks through the call ------------------------------------------------------------------------------

def test_blocks_mixed_encoders(codec):
    """One hpack.encode_blocks call whose encoders are Huffman-coding and not, mixed, with blocks of indexed
    headers only and an empty block: every block is hpack_ref.Encoder's, per encoder."""
    from test_hpack_encoder import response_lists

    from loona_amd import hpack

    lists = response_lists(seed=7, n=120)
    lists[3] = []  # an empty block
    lists[10] = [(b":status", b"200"), (b":method", b"GET")]  # static-table hits only: no string at all
    lists[11] = list(lists[10])
    k = 4
    encs = [hpack.Encoder(huffman=bool(i % 2)) for i in range(k)]
    refs = [hpack_ref.Encoder(huffman=bool(i % 2)) for i in range(k)]
    got = hpack.encode_blocks([(encs[i % k], hs) for i, hs in enumerate(lists)], codec)
    want = [refs[i % k].encode(hs) for i, hs in enumerate(lists)]
    assert got == want and got[3] == b"" and got[10] == bytes([0x88, 0x82])
    # the encoders took their tables: a second call indexes what the first one added
    got = hpack.encode_blocks([(encs[i % k], hs) for i, hs in enumerate(lists)], codec)
    assert got == [refs[i % k].encode(hs) for i, hs in enumerate(lists)]
