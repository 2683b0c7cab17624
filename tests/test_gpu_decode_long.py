"""The long-literal and the huge-literal phase at their placed edges, against the C oracle bit for bit: no tolerance.

The cases come from decode_long_cases.py, which places them against the kernels' own constants
(hpk_test_decode_geometry); test_decode_long_cases.py proves on the CPU that each reaches the edge it is named
for. Every case goes through the C ABI with the wave kernel and the workgroup-fill kernel forced: the region form
with the input at +0 and +5 from a 16-byte boundary (regions of the decoded bound back to back, or the case's own
capacities), the compacted form, and, all cases in one batch, the packed form. One checker serves the region
form: the output is guard | regions | guard, all 0xAB, out_len and status prefilled with values the kernels never
write; afterwards every literal has the oracle's status and length (HPK_OUTPUT_OVERFLOW and the capacity where the
region is smaller than the decoded size), the oracle's bytes below out_len, and no byte outside the regions has
changed. Bytes of a region past out_len are unspecified (hpk.h) and not looked at."""

import time

import numpy as np
import pytest

import decode_long_cases as dc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 4096
FILL = 0xAB
KERNELS = ("wave", "fill")
SHIFTS = ((0, 0), (5, 3))  # (input, output) bytes past a 16-byte boundary
FAMILIES = ("noresync-", "none-chain-", "straddle30-", "straddle13-", "pair-on-boundary-", "eos-at-", "last-piece-",
            "terminal-early", "ov-pb", "share-", "huge-capacity-", "long-sweep", "long-ring", "long-short-output",
            "long-tail", "long-claims-dense-", "long-claims-sprinkled-", "long-capacity-")
STATUS_BUILT_IN = ("none-chain-", "straddle30-", "straddle13-", "eos-at-", "terminal-early")


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU)")
    from loona_amd import HuffmanCodec

    c = HuffmanCodec(0, stream=torch.cuda.current_stream())
    yield c
    c.close()


@pytest.fixture(scope="module")
def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def off_dev(a):
    return to_dev(np.asarray(a, np.int64).astype(np.uint32).view(np.int32))


def dev_input(blob, in_shift, behind=b""):
    """the blob on the device, `in_shift` bytes past a 16-byte boundary, `behind` right after it: the tensor
    handed to the call ends with the blob (in_cap = its size)"""
    src = np.zeros(in_shift + blob.size + len(behind), np.uint8)
    src[in_shift : in_shift + blob.size] = blob
    src[in_shift + blob.size :] = np.frombuffer(behind, np.uint8)
    return to_dev(src)[in_shift : in_shift + blob.size]


def decode_regions(codec, blob_dev, in_off, out_off, out_shift):
    """hpk_decode_batch into guard | regions | guard: (region bytes, out_len, status), guards checked"""
    n, total = len(in_off) - 1, int(out_off[-1])
    lead = GUARD + out_shift
    big = torch.full((lead + total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    ol = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    codec.decode_into(blob_dev, off_dev(in_off), big[lead : lead + total], off_dev(out_off), ol, st, device=True, sync=True)
    g = big.cpu().numpy()
    assert (g[:lead] == FILL).all(), "bytes before the first region changed"
    assert (g[lead + total :] == FILL).all(), "bytes at or past the last region's end changed"
    return g[lead : lead + total], ol.cpu().numpy().astype(np.int64), st.cpu().numpy()


def assert_same(x, out, starts, ol, st, what):
    bad = np.nonzero(st != x.status)[0]
    assert bad.size == 0, f"{what}: status differs at {bad[:10]}: {st[bad[:10]]} for {x.status[bad[:10]]}"
    bad = np.nonzero(ol != x.out_len)[0]
    assert bad.size == 0, f"{what}: out_len differs at {bad[:10]}: {ol[bad[:10]]} for {x.out_len[bad[:10]]}"
    got = dc.gather(out, starts, x.out_len)
    if not np.array_equal(got, x.flat):
        first = int(np.nonzero(got != x.flat)[0][0])
        lit = int(np.searchsorted(np.cumsum(x.out_len), first, side="right"))
        raise AssertionError(f"{what}: decoded bytes differ, first in literal {lit} of {len(ol)} (input bytes "
                             f"{x.in_off[lit]}..{x.in_off[lit + 1]}), at its byte {first - int(x.out_len[:lit].sum())}")


def check_region(codec, x, in_shift, out_shift, what):
    out, ol, st = decode_regions(codec, dev_input(x.blob, in_shift), x.in_off, x.out_off, out_shift)
    assert_same(x, out, x.out_off, ol, st, what)


def check_compact(codec, x, what):
    """hpk_decode_batch_compact: every literal's bytes, length and status; nothing outside [0, out_off[n])"""
    from loona_amd.batch import compact_capacity

    n = len(x.in_off) - 1
    need = compact_capacity(int(x.blob.size), n)
    big = torch.full((GUARD + need + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    _, oo, ol, st = codec.decode_compact(dev_input(x.blob, 0), off_dev(x.in_off), out_blob=big[GUARD : GUARD + need], sync=True)
    g = big.cpu().numpy()
    o = oo.cpu().numpy().astype(np.uint32).astype(np.int64)
    assert int(o[n]) <= need, what
    assert_same(x, g[GUARD : GUARD + need], o[:n], ol[:n].cpu().numpy().astype(np.uint32).astype(np.int64), st[:n].cpu().numpy(),
                what)
    assert (g[:GUARD] == FILL).all(), f"{what}: bytes written before the output"
    assert (g[GUARD + int(o[n]) :] == FILL).all(), f"{what}: bytes written past the reported span"


def expected(name, cus):
    c = dc.case(name, cus)
    x = dc.expected_of(name, cus)
    if name.startswith(STATUS_BUILT_IN):  # the status the case was built for, besides equality with the oracle
        assert x.status[0] == c.meta["status"], name
    return c, x


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("family", FAMILIES)
def test_region_form(codec, cus, family, kernel):
    codec.set_decode_kernel(kernel)
    t0 = time.perf_counter()
    for name in dc.names(family):
        _, x = expected(name, cus)
        for in_shift, out_shift in SHIFTS:
            check_region(codec, x, in_shift, out_shift, f"{name}, {kernel} kernel, input +{in_shift}, output +{out_shift}")
    print(f"\n{family}* ({kernel}): {len(dc.names(family))} cases x {len(SHIFTS)} calls, {(time.perf_counter() - t0) * 1e3:.1f} ms")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("family", [f for f in FAMILIES if "capacity" not in f])
def test_compact_form(codec, cus, family, kernel):
    codec.set_decode_kernel(kernel)
    for name in dc.names(family):
        _, x = expected(name, cus)
        check_compact(codec, x, f"{name}, {kernel} kernel, compacted form")


def test_packed_form_all_cases_at_once(codec, cus):
    """hpk_decode_batch_packed on one batch that holds every case (but those with capacities of their own, which
    the packed form has no say in): out_off the exclusive sum of the oracle's lengths, the bytes end to end"""
    codec.set_decode_kernel("auto")
    names = [n for n in dc.CASE_NAMES if "capacity" not in n]
    xs = [dc.expected_of(n, cus) for n in names]
    blob = np.concatenate([x.blob for x in xs])
    lens = np.concatenate([np.diff(x.in_off) for x in xs])
    io = np.concatenate([[0], np.cumsum(lens)])
    want_len = np.concatenate([x.out_len for x in xs])
    want_st = np.concatenate([x.status for x in xs])
    flat = np.concatenate([x.flat for x in xs])
    n, total = len(lens), int(want_len.sum())
    big = torch.full((GUARD + total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    _, po, pl, pst = codec.decode_packed(to_dev(blob), off_dev(io), out_blob=big[GUARD : GUARD + total], sync=True)
    g = big.cpu().numpy()
    assert np.array_equal(pst[:n].cpu().numpy(), want_st), "packed form: status"
    assert np.array_equal(pl[:n].cpu().numpy().astype(np.uint32).astype(np.int64), want_len), "packed form: out_len"
    assert np.array_equal(po.cpu().numpy().astype(np.uint32).astype(np.int64), np.concatenate([[0], np.cumsum(want_len)]))
    assert np.array_equal(g[GUARD : GUARD + total], flat), "packed form: bytes"
    assert (g[:GUARD] == FILL).all() and (g[GUARD + total :] == FILL).all(), "packed form: bytes outside the output changed"


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", dc.names("neighbour-bytes-"))
def test_neighbour_bytes(codec, name, kernel):
    """The last literal of a batch that ends at in_cap, in_cap mod 16 = 1 or 15: whatever the caller's buffer holds
    behind in_cap and whatever the last byte of the literal in front is, its length, status and bytes are the
    oracle's."""
    codec.set_decode_kernel(kernel)
    c = dc.case(name)
    x = dc.expected_of(name)
    assert x.status[1] == c.meta["status"] and x.blob.size % 16 in (1, 15)
    a, b = int(x.out_len[0]), int(x.out_len[0] + x.out_len[1])
    seen = set()
    for front_last in (0x00, 0xFF):
        for behind in (0x00, 0xFF):
            blob = x.blob.copy()
            blob[x.in_off[1] - 1] = front_last
            out, ol, st = decode_regions(codec, dev_input(blob, 0, bytes([behind]) * 64), x.in_off, x.out_off, 0)
            what = f"{name}, {kernel} kernel, front literal ends in {front_last:#x}, {behind:#x} behind in_cap"
            assert (st[1], ol[1]) == (x.status[1], x.out_len[1]), what
            got = out[x.out_off[1] : x.out_off[1] + ol[1]]
            assert np.array_equal(got, x.flat[a:b]), what
            seen.add((int(st[1]), int(ol[1]), got.tobytes()))
    assert len(seen) == 1
