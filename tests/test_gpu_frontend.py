"""GPU parity of the wave fills' front end (decode v40): the fit count, the counting sort and its queue, the
hand-over from one fill to the next and the split write-back, through the C ABI against the library's own CPU
batch path (hpk_decode_batch_cpu). out_len, status and the bytes below out_len must be equal, exactly, with the
wave kernel forced, in the region form and in the compacted form.

  boundaries  1, 2, 63, 64, 65, 107, 108, 127, 128, 129, 193 and 300 config-2 literals (one slot, one lane row, a
              typical fill of ~108, a full fill of 128 and one past each), and 97 (one past a 96-literal chunk);
              and 33,000, the least batch whose workgroup ranges (one per CU, 256 of them) pass 128 literals, so
              that a wave takes a whole 96-literal chunk in one fill and both of a lane's slots are used (a
              smaller batch runs on one workgroup per 64 literals);
  classes     128 literals of one encoded length (one class takes every atomic); encoded lengths 0, 1, 2, 3 mixed
              with 62 and 63 (classes 0 and 31, empty literals); a strictly increasing and a strictly decreasing
              run of lengths;
  kq < k      every third literal >= 64 encoded bytes (listed for the long phase); some regions one byte below the
              decoded bound (the byte path); one fill of only such literals (kq == 0 for the lane walk);
  image       300 literals of 40 five-bit-code symbols in bound-sized regions, and the config-2 literals with 64
              bytes of slack in every region, where the image cuts the fill at a few dozen literals;
  errors      400 literals with in_off non-monotone at literal 150 and, separately, at literal 96 (literal 0 of the
              second 96-literal chunk); out_off past out_cap from the same two literals on;
  guided      one device-generated batch of 4M + 129 literals (the guided hand-out), checked against its strings.

The error cases, as the parent commit's library (decode v39) returns them on an MI355X, recorded once from that
library: a batch of 400 literals runs on 7 workgroups, workgroup b taking literals [400 b / 7, 400 (b + 1) / 7), each
range one wave's single fill. in_off decreasing at literal 150 (in_off[150] = in_off[151] + 3): HPK_BAD_OFFSETS and
out_len 0 on [114, 171), the range of workgroup 2, and nothing else. At literal 96: on [57, 114), workgroup 1's range
(literal 95's end offset is the bad one). out_off past out_cap from literal 150 on: [114, 400); from literal 96 on:
[57, 400). Every other literal as the CPU path's (the literal right before a moved in_off, whose input grew, lies
in the bad range both times). The compacted form returns the same two ranges for the moved in_off; it makes its own
regions, and refuses an out_cap below its bound before any launch (HPK_E_INVAL)."""


import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT = 0xAB
GUARD = 256
FIVE = np.frombuffer(b"012aceiost", np.uint8)  # the ten 5-bit codes of RFC 7541 Appendix B


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU)")
    from loona_amd import HuffmanCodec

    c = HuffmanCodec(0, stream=torch.cuda.current_stream())
    c.set_decode_kernel("wave")
    yield c
    c.close()


_c2 = None


def _config2(k):
    """The first k literals of one 33,000-literal config-2 batch (made once)."""
    global _c2
    from loona_amd import synth

    if _c2 is None:
        w = synth.config2(n=33000)
        _c2 = [w.enc_blob[w.enc_off[i] : w.enc_off[i + 1]].tobytes() for i in range(w.n)]
    return _c2[:k]


def _lit5(rng, nbytes):
    """A literal of exactly nbytes encoded bytes whose decoded length is its decoded bound floor(8 nbytes / 5)."""
    from loona_amd import huffman_encode

    e = huffman_encode(rng.choice(FIVE, (8 * nbytes) // 5).tobytes())
    assert len(e) == nbytes
    return e


def _bound(off):
    return (np.diff(off.astype(np.int64)) * 8) // 5


def _case(name):
    """(literals, region sizes) of a named case; the regions are the decoded bounds unless the case says otherwise."""
    from hpk_util import pack

    rng = np.random.default_rng(4000 + sum(name.encode()))
    if name.startswith("c2_"):
        lits = _config2(int(name[3:]))
    elif name == "one_class":
        lits = [_lit5(rng, 24) for _ in range(128)]
    elif name == "classes_0_31":
        lits = [_lit5(rng, [0, 1, 2, 3, 62, 63][int(rng.integers(0, 6))]) for _ in range(128)]
    elif name == "increasing":
        lits = [_lit5(rng, k) for k in range(64)]
    elif name == "decreasing":
        lits = [_lit5(rng, 63 - k) for k in range(64)]
    elif name == "third_long":
        lits = [_lit5(rng, int(rng.integers(64, 120))) if i % 3 == 2 else x for i, x in enumerate(_config2(240))]
    elif name == "some_below_bound":
        lits = [_lit5(rng, int(rng.integers(5, 40))) if i % 7 == 3 else x for i, x in enumerate(_config2(240))]
    elif name == "all_below_bound":
        lits = [_lit5(rng, int(rng.integers(5, 40))) if i % 4 == 1 else x for i, x in enumerate(_config2(100))]
    elif name == "five_bit_300":
        lits = [_lit5(rng, 25) for _ in range(300)]
    elif name == "slack_64":
        lits = _config2(300)
    else:
        raise KeyError(name)
    blob, off = pack(lits)
    cap = _bound(off)
    if name == "some_below_bound":  # every fifth region one byte short: the 5-bit literals among them overflow
        cap[::5] = np.maximum(cap[::5] - 1, 0)
    elif name == "all_below_bound":  # (the 5-bit literals overflow, the config-2 ones fit)
        cap = np.maximum(cap - 1, 0)
    elif name == "slack_64":
        cap = cap + 64
    return blob, off, cap


CASES = ["c2_%d" % k for k in (1, 2, 63, 64, 65, 97, 107, 108, 127, 128, 129, 193, 300, 33000)] + [
    "one_class", "classes_0_31", "increasing", "decreasing", "third_long", "some_below_bound", "all_below_bound",
    "five_bit_300", "slack_64"]


def _cpu(blob, in_off, oo):
    """hpk_decode_batch_cpu on the caller's regions: (out_blob, out_off, out_len, status)."""
    from loona_amd import _lib

    n = len(in_off) - 1
    in_off = np.ascontiguousarray(in_off, np.uint32)
    oo = np.ascontiguousarray(oo, np.uint32)
    out = np.zeros(max(int(oo[-1]), 1), np.uint8)
    ol = np.zeros(max(n, 1), np.uint32)
    st = np.zeros(max(n, 1), np.uint8)
    src = blob if blob.size else np.zeros(1, np.uint8)
    rc = _lib.lib().hpk_decode_batch_cpu(src.ctypes.data, in_off.ctypes.data, n, out.ctypes.data, oo.ctypes.data,
                                         ol.ctypes.data, st.ctypes.data, 1)
    assert rc == 0
    return out, oo, ol[:n], st[:n]


def _offsets(cap):
    oo = np.zeros(len(cap) + 1, np.int64)
    np.cumsum(cap, out=oo[1:])
    return oo


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _region(codec, blob, in_off_dev, oo, out_cap=None, shift=3):
    """The region form on an unaligned base between guard bytes: (bytes, out_len, status, the call's error)."""
    n = len(oo) - 1
    span = int(oo[-1]) if out_cap is None else out_cap
    big = torch.full((GUARD + shift + span + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    out = big[GUARD + shift : GUARD + shift + max(span, 1)]
    ol = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    err = None
    src = _dev(blob) if blob.size else torch.zeros(1, dtype=torch.uint8, device="cuda")
    try:
        codec.decode_into(src, in_off_dev, out, _dev(oo.astype(np.uint32).view(np.int32)), ol, st, device=True, sync=True)
    except RuntimeError as e:
        err = e
    g = big.cpu().numpy()
    assert (g[: GUARD + shift] == SENT).all(), "bytes written before the output"
    assert (g[GUARD + shift + span :] == SENT).all(), "bytes written past the output"
    return g[GUARD + shift : GUARD + shift + span], ol.cpu().numpy().astype(np.uint32), st.cpu().numpy(), err


def _same(got, want, idx, what):
    """out_len, status and the bytes below out_len of the literals idx: (bytes, out_off, out_len, status) pairs."""
    go, goo, gl, gs = got
    wo, woo, wl, ws = want
    idx = np.asarray(idx, np.int64)
    bad = idx[gs[idx] != ws[idx]]
    assert bad.size == 0, f"{what}: status differs at {bad[:8]}: {gs[bad[:8]]} vs {ws[bad[:8]]}"
    bad = idx[gl[idx] != wl[idx]]
    assert bad.size == 0, f"{what}: out_len differs at {bad[:8]}: {gl[bad[:8]]} vs {wl[bad[:8]]}"
    for i in idx:
        a, b, ln = int(goo[i]), int(woo[i]), int(wl[i])
        assert np.array_equal(go[a : a + ln], wo[b : b + ln]), f"{what}: bytes of literal {i} differ"


@pytest.mark.parametrize("name", CASES)
def test_frontend_region_form(codec, name):
    blob, off, cap = _case(name)
    oo = _offsets(cap)
    want = _cpu(blob, off, oo)
    outn, ol, st, err = _region(codec, blob, _dev(off.astype(np.int32)), oo)
    assert err is None, err
    if name.endswith("below_bound"):
        assert (want[3] == 4).any() and (want[3] == 0).any(), "the case holds overflowing and fitting literals"
    _same((outn, oo, ol, st), want, np.arange(len(cap)), f"region form, {name}")


@pytest.mark.parametrize("name", CASES)
def test_frontend_compact_form(codec, name):
    """The compacted form lays its own regions out (the decoded bounds, 4-rounded): against the CPU path on the
    decoded bounds; nothing outside [0, out_off[n]) is written and no two literals overlap."""
    from loona_amd.batch import compact_capacity

    blob, off, _ = _case(name)
    n = len(off) - 1
    want = _cpu(blob, off, _offsets(_bound(off)))
    need = compact_capacity(int(blob.size), n)
    big = torch.full((GUARD + need + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    src = _dev(blob) if blob.size else torch.zeros(1, dtype=torch.uint8, device="cuda")
    _, oo, ol, st = codec.decode_compact(src, _dev(off.astype(np.int32)), out_blob=big[GUARD : GUARD + max(need, 1)],
                                         sync=True)
    g = big.cpu().numpy()
    o = oo.cpu().numpy().astype(np.uint32)
    end = int(o[n])
    assert end <= need
    got = (g[GUARD : GUARD + need], o, ol[:n].cpu().numpy().astype(np.uint32), st[:n].cpu().numpy())
    _same(got, want, np.arange(n), f"compacted form, {name}")
    assert (g[:GUARD] == SENT).all(), "bytes written before the output"
    assert (g[GUARD + end :] == SENT).all(), "bytes written past the reported span"
    ln = got[2].astype(np.int64)
    s = o[:n].astype(np.int64)[ln > 0]
    e = s + ln[ln > 0]
    order = np.argsort(s)
    assert (s[order][1:] >= e[order][:-1]).all(), "compacted literals overlap"


# ---- errors across the hand-over (the expected ranges: the module docstring) ----
ERR_N = 400
BAD_IN = {150: (114, 171), 96: (57, 114)}
BAD_OUT = {150: (114, 400), 96: (57, 400)}


def _err_batch():
    from hpk_util import pack

    blob, off = pack(_config2(ERR_N))
    oo = _offsets(_bound(off))
    return blob, off, oo, _cpu(blob, off, oo)


def _check_bad(outn, oo, ol, st, want, lo, hi, also_off, what):
    from loona_amd import _lib

    idx = np.arange(ERR_N)
    bad = (idx >= lo) & (idx < hi)
    assert (st[bad] == _lib.HPK_BAD_OFFSETS).all() and (ol[bad] == 0).all(), f"{what}: the bad range [{lo}, {hi})"
    assert not (st[~bad] == _lib.HPK_BAD_OFFSETS).any(), f"{what}: HPK_BAD_OFFSETS outside [{lo}, {hi})"
    good = ~bad
    for i in also_off:
        good[i] = False
    _same((outn, oo, ol, st), want, idx[good], what)


@pytest.mark.parametrize("j", [150, 96])
def test_frontend_in_off_not_monotone(codec, j):
    blob, off, oo, want = _err_batch()
    io = off.astype(np.int64).copy()
    io[j] = io[j + 1] + 3
    outn, ol, st, err = _region(codec, blob, _dev(io.astype(np.uint32).view(np.int32)), oo)
    assert err is not None and "hpk_decode_batch" in str(err)
    lo, hi = BAD_IN[j]
    _check_bad(outn, oo, ol, st, want, lo, hi, [j - 1], f"in_off decreasing at {j}, region form")
    # the compacted form: the same literals are refused (its regions come from in_off), the others as the CPU path's
    from loona_amd.batch import compact_capacity

    need = compact_capacity(int(blob.size), ERR_N)
    big = torch.full((need + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    cerr = None
    oo_c = torch.zeros(ERR_N + 1, dtype=torch.int32, device="cuda")
    ol_c = torch.full((ERR_N,), 7, dtype=torch.int32, device="cuda")
    st_c = torch.full((ERR_N,), 9, dtype=torch.uint8, device="cuda")
    try:
        codec.decode_compact(_dev(blob), _dev(io.astype(np.uint32).view(np.int32)), out_blob=big[:need], out_off=oo_c,
                             out_len=ol_c, status=st_c, sync=True)
    except RuntimeError as e:
        cerr = e
    assert cerr is not None
    g = big.cpu().numpy()
    assert (g[need:] == SENT).all(), "bytes written past the output"
    got = (g[:need], oo_c.cpu().numpy().astype(np.uint32), ol_c.cpu().numpy().astype(np.uint32), st_c.cpu().numpy())
    _check_bad(got[0], got[1], got[2], got[3], want, lo, hi, [j - 1], f"in_off decreasing at {j}, compacted form")


@pytest.mark.parametrize("j", [150, 96])
def test_frontend_out_off_past_out_cap(codec, j):
    blob, off, oo, want = _err_batch()
    cap = int(oo[j + 1]) - 1  # literal j's region ends one byte past the output
    outn, ol, st, err = _region(codec, blob, _dev(off.astype(np.int32)), oo, out_cap=cap)
    assert err is not None and "hpk_decode_batch" in str(err)
    lo, hi = BAD_OUT[j]
    _check_bad(outn, oo, ol, st, want, lo, hi, [], f"out_off past out_cap from {j}, region form")
    # the compacted form refuses a capacity below its bound before any launch
    big = torch.full((cap + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):
        codec.decode_compact(_dev(blob), _dev(off.astype(np.int32)), out_blob=big[:cap], sync=True)
    assert (big.cpu().numpy() == SENT).all(), "the refused call wrote"


def test_frontend_guided_hand_out(codec):
    """4M + 129 device-generated config-2 literals: the guided hand-out (chunks of 1/32 of what is left), region and
    compacted form against the generated strings."""
    from loona_amd import synth
    from loona_amd.batch import decode_offsets_torch

    w = synth.device_config2(codec, n=4_000_129)
    doff = decode_offsets_torch(w.enc_off)
    out = torch.empty(int(doff[-1].item()) + 16, dtype=torch.uint8, device="cuda")
    ol = torch.empty(w.n, dtype=torch.int32, device="cuda")
    st = torch.empty(w.n, dtype=torch.uint8, device="cuda")
    codec.decode_into(w.enc_blob, w.enc_off, out, doff, ol, st, device=True, sync=True)
    synth.check_decoded(w, out, doff, ol, st)
    del out
    out, oo, ol, st = codec.decode_compact(w.enc_blob, w.enc_off, sync=True)
    synth.check_decoded(w, out, oo, ol, st)
