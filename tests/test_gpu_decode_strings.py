"""The packed string-literal decode on the GPU (hpk_decode_strings_packed), byte for byte: no tolerance. The
expected result is decode_strings_cases.expected(): hpack_ref.decode_integer's prefix, decode_string's length
check and the C oracle's Huffman decode (partial bytes kept), proven equal to hpack_ref.decode_string window by
window in test_decode_strings_cases.py; never the code under test.

One checker serves every case, in the shape of test_gpu_encode_strings.check: the output view sits `out_shift`
bytes into a canary-filled buffer with 4 KiB guards on both sides; out_off, out_len, consumed and status are
prefilled with values the call never writes; afterwards they are the expected ones, the bytes below
min(total, cap) are the expected ones, and the canary is intact at and past that point and in both guards. Every
case whose windows lie end to end runs in the mirror form (str_end = None, n + 1 offsets) and in the explicit form
with every window extended to the blob's end (the reference's "rest of the block"), each against its own expected
answer. Three kinds of case differ: the run of empty and void strings takes the explicit form with the mirror
form's windows (extended, its void strings would read their neighbours); the void, shared and overlapping windows
of section 8 are built for one form each (a decreasing pair exists only in the mirror form, str_off > str_end only
in the explicit one); and the round trip and the equivalence test also call the mirror form directly."""

import ctypes

import numpy as np
import pytest

import decode_strings_cases as dc
from hpk_util import pack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CANARY = 0xA5
GUARD = 4096
PRE_OFF, PRE_LEN, PRE_CON, PRE_ST = -3, 7, 11, 9


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU)")
    from loona_amd import HuffmanCodec

    c = HuffmanCodec(0, stream=torch.cuda.current_stream())
    yield c
    c.close()


@pytest.fixture(scope="module")
def geometry():
    from loona_amd import _lib

    t, l = ctypes.c_uint32(0), ctypes.c_uint32(0)
    assert _lib.lib().hpk_test_pack_geometry(ctypes.byref(t), ctypes.byref(l)) == _lib.HPK_E_OK
    return t.value, l.value


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def off_dev(a):
    return to_dev(np.asarray(a, np.int64).astype(np.uint32).view(np.int32))


def dev_input(blob, in_shift, in_cap=None):
    src = np.zeros(in_shift + blob.size + 1, np.uint8)
    src[in_shift : in_shift + blob.size] = blob
    return to_dev(src)[in_shift : in_shift + (blob.size if in_cap is None else in_cap)]


def mirror_offsets(b):
    """the n + 1 offsets of a batch whose windows lie end to end"""
    n = len(b.str_off)
    assert n == 0 or np.array_equal(b.str_off[1:], b.str_end[:-1])
    return np.append(b.str_off, b.str_end[-1] if n else 0)


def run(codec, blob, str_off, str_end, in_shift, out_shift, cap, sync=True, raises=None, in_cap=None):
    """decode_strings into a view of `cap` bytes -> (view, out_off, out_len, consumed, status, guards)"""
    n = len(str_off) - (1 if str_end is None else 0)
    dblob = dev_input(blob, in_shift, in_cap)
    doff, dend = off_dev(str_off), None if str_end is None else off_dev(str_end)
    big = torch.full((GUARD + out_shift + cap + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    view = big[GUARD + out_shift : GUARD + out_shift + cap]
    oo = torch.full((n + 1,), PRE_OFF, dtype=torch.int32, device="cuda")
    ol = torch.full((max(n, 1),), PRE_LEN, dtype=torch.int32, device="cuda")
    co = torch.full((max(n, 1),), PRE_CON, dtype=torch.int32, device="cuda")
    st = torch.full((max(n, 1),), PRE_ST, dtype=torch.uint8, device="cuda")
    kw = dict(out_blob=view, out_off=oo, out_len=ol, consumed=co, status=st)
    if raises is None:
        codec.decode_strings(dblob, doff, dend, sync=sync, **kw)
        if not sync:
            codec.check()
    else:
        with pytest.raises(RuntimeError, match=raises):
            codec.decode_strings(dblob, doff, dend, sync=True, **kw)
    torch.cuda.synchronize()
    g = big.cpu().numpy()
    lead = GUARD + out_shift
    u = lambda t: t.cpu().numpy().view(np.uint32).astype(np.int64)  # noqa: E731
    return g[lead : lead + cap], u(oo), u(ol)[:n], u(co)[:n], st[:n].cpu().numpy(), (g[:lead], g[lead + cap :])


def compare(what, x, got, cap):
    view, oo, ol, co, st, guards = got
    n, total = len(x.out_len), int(x.out_off[-1])
    bad = np.nonzero(st != x.status)[0]
    assert bad.size == 0, f"{what}: status differs at {bad[:10]}: {st[bad[:10]]} for {x.status[bad[:10]]}"
    bad = np.nonzero(ol != x.out_len)[0]
    assert bad.size == 0, f"{what}: out_len differs at {bad[:10]}: {ol[bad[:10]]} for {x.out_len[bad[:10]]}"
    bad = np.nonzero(co != x.consumed)[0]
    assert bad.size == 0, f"{what}: consumed differs at {bad[:10]}: {co[bad[:10]]} for {x.consumed[bad[:10]]}"
    assert np.array_equal(oo, x.out_off), f"{what}: out_off is not the exclusive sum of the expected lengths"
    k = min(total, cap)
    if not np.array_equal(view[:k], x.flat[:k]):
        first = int(np.nonzero(view[:k] != x.flat[:k])[0][0])
        s = int(np.searchsorted(x.out_off, first, "right")) - 1
        raise AssertionError(f"{what}: bytes differ first at {first} (string {s} of {n}, Huffman {bool(x.huff[s])}, payload "
                             f"{x.pay_off[s]}+{x.pay_len[s]}, output {x.out_off[s]}..{x.out_off[s + 1]}): "
                             f"{view[first]:#x} for {x.flat[first]:#x}")
    assert (view[k:] == CANARY).all(), f"{what}: bytes at or past out_off[n] were written"
    assert (guards[0] == CANARY).all() and (guards[1] == CANARY).all(), f"{what}: bytes outside the output view were written"


def check(codec, b, what, in_shift=0, out_shift=0, cap=None, sync=True, raises=None, forms=("mirror", "to_end"), x=None):
    """A batch whose windows lie end to end, in the mirror form and in the explicit form with every window
    extended to the blob's end ("explicit" instead of "to_end": str_end given, the windows the mirror form's, for a
    batch whose case depends on where its windows end); cap: the output view's bytes (default: the total; an int,
    or a function of the total)."""
    out = {}
    for form in forms:
        if form == "mirror":
            xe = dc.expected(b) if x is None else x
            off, end = mirror_offsets(b), None
        elif form == "explicit":  # str_end given, the windows the mirror form's
            xe = dc.expected(b) if x is None else x
            off, end = b.str_off, b.str_end
        else:
            e = dc.to_end(b)
            xe = dc.expected(e)
            assert int(xe.pay_len[xe.huff].sum()) <= b.blob.size, f"{what}: the to-end form's Huffman payloads pass the blob"
            off, end = e.str_off, e.str_end
        total = int(xe.out_off[-1])
        c = total if cap is None else cap(total) if callable(cap) else cap
        r = raises(total, c) if callable(raises) else raises
        got = run(codec, b.blob, off, end, in_shift, out_shift, c, sync, r)
        compare(f"{what} ({form})", xe, got, c)
        out[form] = xe
    return out


# ---- 1. round trip ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def strs():
    return dc.round_trip_strings()


@pytest.mark.parametrize("policy", ["auto", "raw", "huffman", "mixed"])
def test_round_trip(codec, strs, policy):
    n = len(strs)
    pol = {"auto": None, "raw": np.full(n, 1, np.uint8), "huffman": np.full(n, 2, np.uint8),
           "mixed": (np.arange(n) % 3).astype(np.uint8)}[policy]
    blob, off = pack(strs)
    eb, eo, el, est = codec.encode_strings(to_dev(blob), off_dev(off), None if pol is None else to_dev(pol), sync=True)
    assert not est[:n].cpu().numpy().any()
    # the encoder's output as it stands: out_off as str_off
    ob, oo, ol, co, st = codec.decode_strings(eb, eo, sync=True)
    assert not st[:n].cpu().numpy().any()
    assert ob.cpu().numpy().tobytes() == b"".join(strs)
    assert torch.equal(co[:n], el[:n]), "consumed is not the encoder's out_len"
    assert np.array_equal(ol[:n].cpu().numpy(), np.diff(off.astype(np.int64)))
    # and through the checker, both forms, against the model
    enc_off = eo.cpu().numpy().view(np.uint32).astype(np.int64)
    b = dc.Batch(eb.cpu().numpy(), enc_off[:-1], enc_off[1:])
    x = check(codec, b, f"round trip {policy}", in_shift=3, out_shift=5, sync=False)
    assert x["mirror"].flat.tobytes() == b"".join(strs)
    if policy == "auto":
        assert x["mirror"].huff.any() and (~x["mirror"].huff & (x["mirror"].pay_len > 0)).any()


# ---- 2. equivalence with decode_packed ----------------------------------------------------------------

def test_all_huffman_equals_decode_packed(codec):
    b, _ = dc.mixed_batch(3000, 37000, raw_share=0.0)
    vec = dc.error_vectors(30)
    b = dc.batch_of([b.blob[a:e].tobytes() for a, e in zip(b.str_off, b.str_end)] + [dc.frame(p, True) for p, _ in vec])
    x = dc.expected(b)
    n = len(b.str_off)
    hb, ho = pack([b.blob[a : a + k].tobytes() for a, k in zip(x.pay_off, x.pay_len)])
    pb, po, pl, pst = codec.decode_packed(to_dev(hb), off_dev(ho), sync=True)
    sb, so, sl, sc_, sst = codec.decode_strings(to_dev(b.blob), off_dev(mirror_offsets(b)), sync=True)
    assert torch.equal(pl[:n], sl[:n]) and torch.equal(pst[:n], sst[:n]) and torch.equal(po, so) and torch.equal(pb, sb)
    assert set(pst[:n].cpu().numpy().tolist()) == {0, 1, 2, 3}


# ---- 3. prefix shapes ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def shapes():
    # (a tail of zeros: the to-end form's windows turn cut integers into long strings, whose Huffman payloads
    # must still sum to no more than the blob)
    return dc.batch_of([w for _, w in dc.prefix_shapes()], tail=bytes(1 << 18))


def test_prefix_shapes(codec, shapes):
    x = check(codec, shapes, "prefix shapes")
    assert {dc.OK, dc.TOO_MANY, dc.INT_SHORT, dc.STR_SHORT} <= set(x["mirror"].status.tolist())
    assert {dc.OK, dc.TOO_MANY, dc.STR_SHORT} <= set(x["to_end"].status.tolist())  # (no window ends inside an integer)
    check(codec, shapes, "prefix shapes, misaligned", in_shift=13, out_shift=7, sync=False)


# ---- 4. Huffman errors inside framed strings --------------------------------------------------------------

def test_huffman_errors_keep_partial_bytes_and_neighbours(codec):
    vec = dc.error_vectors(200)
    wins = []
    for i, (p, _) in enumerate(vec):
        wins.append(dc.frame(p, True))
        wins.append(dc.frame_plain(b"neighbour-%d" % i, i % 2 == 0))
    b = dc.batch_of(wins)
    x = check(codec, b, "Huffman errors")["mirror"]
    assert np.array_equal(x.status[0::2], [s for _, s in vec]) and not x.status[1::2].any()
    assert (x.consumed[0::2] == b.str_end[0::2] - b.str_off[0::2]).all() and x.out_len[0::2].sum() > 0
    check(codec, b, "Huffman errors, misaligned", in_shift=1, out_shift=15, x=x)


# ---- 5. placed pack cases -----------------------------------------------------------------------------

@pytest.mark.parametrize("out_shift", [0, 1, 15])
def test_alternating_sources_in_every_chunk(codec, out_shift):
    check(codec, dc.alternating(), "alternating raw/Huffman", in_shift=out_shift, out_shift=out_shift)


def test_empties_pass_the_window(codec, geometry):
    b = dc.empties_then_one(geometry[1])
    # (the explicit form with the mirror form's windows: extended to the blob's end, the void strings of the run
    # would read their neighbours' octets and the run would no longer be empty)
    check(codec, b, "empty and void strings past the LDS window", forms=("mirror", "explicit"))
    check(codec, b, "empty and void strings past the LDS window, misaligned", in_shift=5, out_shift=9,
          forms=("mirror", "explicit"))


def test_raw_string_longer_than_a_tile(codec, geometry):
    b = dc.long_raw(geometry[0])
    for shift in (0, 1, 15):
        check(codec, b, f"raw string of a tile + 17, shift {shift}", in_shift=15 - shift, out_shift=shift)


@pytest.fixture(scope="module")
def mixed3000():
    b, _ = dc.mixed_batch(3000, 38000)
    return b, dc.expected(b)


@pytest.mark.parametrize("in_shift", [0, 1, 15])
@pytest.mark.parametrize("out_shift", [0, 1, 15])
def test_misalignment(codec, mixed3000, in_shift, out_shift):
    b, x = mixed3000
    check(codec, b, f"misaligned in{in_shift} out{out_shift}", in_shift=in_shift, out_shift=out_shift, x=x)


# ---- 6. sizes ---------------------------------------------------------------------------------------------

def test_long_and_huge_payloads(codec):
    check(codec, dc.sizes_batch(), "payloads of 63, 64, 113 bytes and 64 KiB")
    check(codec, dc.sizes_batch(), "payloads of 63, 64, 113 bytes and 64 KiB, misaligned", in_shift=7, out_shift=3,
          sync=False)


@pytest.mark.parametrize("raw_share", [0.0, 1.0], ids=["all-huffman", "all-raw"])
def test_one_form_only(codec, raw_share):
    b, strs = dc.mixed_batch(2500, 39000, raw_share=raw_share)
    x = check(codec, b, f"raw share {raw_share}", out_shift=3)["mirror"]
    assert x.flat.tobytes() == b"".join(strs) and x.huff[x.pay_len > 0].all() == (raw_share == 0.0)


def test_n0_and_n1(codec):
    x = check(codec, dc.batch_of([]), "n = 0")["mirror"]
    assert x.out_off.tolist() == [0]
    check(codec, dc.batch_of([]), "n = 0, room", cap=40, out_shift=5)
    for w in (dc.frame_plain(b"www.example.com", True), dc.frame(b"raw", False), b"\x00", b"\x80", b"", b"\x7f"):
        check(codec, dc.batch_of([w]), f"n = 1 ({w[:4].hex()})", cap=lambda t: t + 3)


def test_just_above_one_workgroup(codec, geometry):
    """n past what one workgroup of each reused kernel takes: the decode's 64 literals per workgroup, the pack's LDS
    window, the scans' 4,096-element tile. Only the pack's window is exported (hpk_test_pack_geometry); the decode's
    grid rule (decode_blocks, hpk_decode.hip: one workgroup per 64 literals) and the scan tile (hpkscan::kTile,
    hpk_scan.h) have no export, so 64 and 4,096 are written here: a change to either moves these cases off their
    edge without failing them, and whoever changes them updates the numbers below."""
    for n in (65, geometry[1] + 1, 4097, 2 * 4096 + 1):
        b, strs = dc.mixed_batch(n, 40000 + n, hi=24)
        x = check(codec, b, f"n = {n}")["mirror"]
        assert x.flat.tobytes() == b"".join(strs)


# ---- 7. capacity ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cut", ["total", "total-1", "0", "total+37"])
def test_capacity(codec, mixed3000, cut):
    b, x = mixed3000
    total = int(x.out_off[-1])
    cap = {"total": total, "total-1": total - 1, "0": 0, "total+37": total + 37}[cut]
    check(codec, b, f"capacity {cut}", out_shift=3, cap=cap, raises="-2" if cap < total else None, x=x)


# ---- 8. offsets -------------------------------------------------------------------------------------------

def test_void_windows_void_only_themselves(codec):
    wins = [dc.frame_plain(b"first-%d" % i, i % 2 == 0) for i in range(40)]
    b = dc.batch_of(wins)
    # the mirror form with one decreasing pair: string 7's window ends before it starts, string 8's spans two
    off = mirror_offsets(b).copy()
    off[8] = off[7] - 2
    m = dc.Batch(b.blob, off[:-1], off[1:])
    x = dc.expected(m)
    assert x.status[7] == dc.BAD_OFFSETS and (np.delete(x.status, 7) != dc.BAD_OFFSETS).all()
    got = run(codec, b.blob, off, None, 0, 3, int(x.out_off[-1]), raises="-1")
    compare("a decreasing pair", x, got, int(x.out_off[-1]))
    # explicit form: str_off > str_end, and an end past in_cap; HPK_E_INVAL wins over HPK_E_NOSPACE
    so, se = b.str_off.copy(), b.str_end.copy()
    so[3], se[3] = se[3], so[3]
    se[11] = b.blob.size + 1
    e = dc.Batch(b.blob, so, se)
    x = dc.expected(e)
    assert np.nonzero(x.status == dc.BAD_OFFSETS)[0].tolist() == [3, 11] and x.out_len[[3, 11]].tolist() == [0, 0]
    total = int(x.out_off[-1])
    for cap in (total, total - 5):
        got = run(codec, b.blob, so, se, 2, 1, cap, raises="-1")
        compare(f"void windows, cap {cap}", x, got, cap)
    # a window inside the allocation but past in_cap is void too
    got = run(codec, b.blob, b.str_off, b.str_end, 0, 0, total + 64, raises="-1", in_cap=b.blob.size - 1)
    x = dc.expected(b, in_cap=b.blob.size - 1)
    assert x.status[-1] == dc.BAD_OFFSETS and not x.status[:-1].any()
    compare("last window past in_cap", x, got, total + 64)
    codec.check()


def test_shared_payload(codec):
    wins = [dc.frame_plain(b"shared-payload-value", True), dc.frame(b"raw-shared", False), dc.frame_plain(b"x", True)]
    b = dc.batch_of(wins, tail=bytes(64))
    so = np.array([b.str_off[0], b.str_off[0], b.str_off[1], b.str_off[1], b.str_off[2]])
    se = np.array([b.str_end[0], b.blob.size, b.str_end[1], b.str_end[1] + 9, b.str_end[2]])
    e = dc.Batch(b.blob, so, se)
    x = dc.expected(e)
    assert not x.status.any() and x.flat.tobytes() == b"shared-payload-value" * 2 + b"raw-shared" * 2 + b"x"
    got = run(codec, b.blob, so, se, 1, 2, int(x.out_off[-1]))
    compare("two strings on one payload", x, got, int(x.out_off[-1]))


def test_overlapping_huffman_payloads_past_in_cap(codec):
    """40 windows on one Huffman string of ~100 bytes: the gathered payloads would pass in_cap. The call refuses
    (HPK_E_INVAL), out_off stays the exclusive sum of out_len, and nothing outside the view is written."""
    s = bytes(np.random.default_rng(41000).choice(np.frombuffer(dc.FIVE_BIT, np.uint8), 160).astype(np.uint8))
    b = dc.batch_of([dc.frame_plain(s, True), dc.frame(b"raw", False)])
    so = np.array([0] * 40 + [int(b.str_off[1])])
    se = np.array([int(b.str_end[0])] * 40 + [int(b.str_end[1])])
    cap = 41 * 160
    view, oo, ol, co, st, guards = run(codec, b.blob, so, se, 0, 5, cap, raises="-1")
    assert np.array_equal(oo, np.concatenate([[0], np.cumsum(ol)]))
    assert (co[:40] == b.str_end[0]).all() and co[40] == 4 and st[40] == 0 and ol[40] == 3
    assert set(st[:40].tolist()) <= {dc.OK, dc.BAD_OFFSETS} and (ol[:40][st[:40] == dc.BAD_OFFSETS] == 0).all()
    good = np.nonzero(st[:40] == 0)[0]
    for i in good:
        assert view[oo[i] : oo[i + 1]].tobytes() == s
    assert (view[oo[-1] :] == CANARY).all() and (guards[0] == CANARY).all() and (guards[1] == CANARY).all()
    codec.check()  # (the flag was taken by the failed call)


# ---- 9. host pointers -------------------------------------------------------------------------------------

def host_call(codec, b, off, end, cap):
    n = len(off) - (1 if end is None else 0)
    buf = np.full(cap + 64, CANARY, np.uint8)
    oo = np.full(n + 1, 0xFFFFFFFD, np.uint32)
    ol = np.full(max(n, 1), PRE_LEN, np.uint32)
    co = np.full(max(n, 1), PRE_CON, np.uint32)
    st = np.full(max(n, 1), PRE_ST, np.uint8)
    blob = np.ascontiguousarray(b.blob)
    args = (blob if blob.size else np.zeros(1, np.uint8)[:0], np.asarray(off, np.int64).astype(np.uint32),
            None if end is None else np.asarray(end, np.int64).astype(np.uint32), buf[:cap], oo, ol, co, st, False, True)
    return args, buf, (oo, ol, co, st)


def host_check(codec, b, what, cap=None, raises=None, forms=("mirror", "to_end")):
    for form in forms:
        e = b if form == "mirror" else dc.to_end(b)
        x = dc.expected(e)
        off, end = (mirror_offsets(b), None) if form == "mirror" else (e.str_off, e.str_end)
        total = int(x.out_off[-1])
        c = total if cap is None else cap(total)
        args, buf, (oo, ol, co, st) = host_call(codec, b, off, end, c)
        r = raises(total, c) if raises else None
        if r is None:
            codec._decode_strings_call(*args)
        else:
            with pytest.raises(RuntimeError, match=r):
                codec._decode_strings_call(*args)
        n = len(x.out_len)
        got = (buf[:c], oo.astype(np.int64), ol[:n].astype(np.int64), co[:n].astype(np.int64), st[:n],
               (buf[c:], np.full(1, CANARY, np.uint8)))
        compare(f"{what} (host, {form})", x, got, c)  # (the bytes at and past min(total, cap) are the canary: exactly
        # that many came back)


def test_host_round_trip(codec, strs):
    blob, off = pack(strs)
    eb, eo, el, est = codec.encode_strings_host(blob, off)
    ob, oo, ol, co, st = codec.decode_strings_host(eb, eo)
    assert not st.any() and ob.tobytes() == b"".join(strs) and np.array_equal(co, el) and ob.size == oo[-1]
    enc = eo.astype(np.int64)
    host_check(codec, dc.Batch(eb, enc[:-1], enc[1:]), "round trip")


def test_host_prefix_shapes(codec, shapes):
    host_check(codec, shapes, "prefix shapes")
    host_check(codec, dc.batch_of([]), "n = 0")


@pytest.mark.parametrize("cut", [0, -1, None, 37])
def test_host_capacity(codec, mixed3000, cut):
    b, _ = mixed3000
    cap = (lambda t: 0) if cut is None else (lambda t: t + cut)
    host_check(codec, b, f"capacity {cut}", cap=cap, raises=lambda t, c: "-2" if c < t else None)


def test_host_bad_offsets_refused_before_any_copy(codec):
    b = dc.batch_of([dc.frame(b"abc", False), dc.frame(b"de", False), dc.frame(b"f", False)])
    off = mirror_offsets(b).copy()
    cases = []
    dec = off.copy()
    dec[2] = dec[1] - 1
    cases.append((dec, None))
    past = off.copy()
    past[-1] = b.blob.size + 1
    cases.append((past, None))
    so, se = b.str_off.copy(), b.str_end.copy()
    so[1], se[1] = se[1], so[1]
    cases.append((so, se))
    for o, e in cases:
        args, buf, (oo, ol, co, st) = host_call(codec, b, o, e, 64)
        with pytest.raises(RuntimeError, match="-1"):
            codec._decode_strings_call(*args)
        assert (buf == CANARY).all() and (oo == 0xFFFFFFFD).all() and (ol == PRE_LEN).all() and (co == PRE_CON).all()
        assert (st == PRE_ST).all()
    codec.check()
