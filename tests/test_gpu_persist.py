"""The small-call mode's persistent kernel (hpk_ctx_set_small_mode) at its placed edges: hpk.h promises "Results are
identical to the launch path's", and this file holds the mode to it, bit for bit, no tolerance.

The batches come from persist_cases.py (test_persist_cases.py proves on the CPU that each holds what its name says;
test_persist_emulation.py replays the per-literal code on the CPU). Every named batch is decoded with the mode on
and compared with the oracle at the same regions and with the launch path (the same call with the mode off):
status, length and valid bytes. The output is guard | blob | guard, all 0xAB, and the canary gaps between regions
(empty literals) are 0xAB too: no guard byte may change, and with the mode on no gap byte (assert_oracle).
hpk_test_small_calls must rise by exactly 1 per call the mode has to answer and by 0 where the launch path has to:
without that a silent fallback hides every bug of the persistent kernel. Further: blob bases at +0, +1 and +15; bad offsets (the declined word against the request
number); input produced on the stream just before the call; an HPK_ASYNC call with the mode on; 1 and 16
workgroups and the argument limits; the request number's wrap at 2^32 (the numbers 0xFFFFFFFF, the kernel's exit
command, and 0, the declined word's idle value, are never issued)."""

import ctypes
import time

import numpy as np
import pytest

import persist_cases as pc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 256
FILL = 0xAB
MODE = (pc.SM_MAX, pc.SM_WGS, pc.SM_IDLE_MS)


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU)")
    from loona_amd import HuffmanCodec

    c = HuffmanCodec(0, stream=torch.cuda.current_stream())
    c.set_small_mode(*MODE)
    yield c
    c.set_small_mode(0)
    c.close()


@pytest.fixture(scope="module")
def L():
    from loona_amd import _lib

    return _lib.lib()


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def off_dev(a):
    return to_dev(np.asarray(a, np.int64).astype(np.uint32).view(np.int32))


def small_calls(L, codec):
    return int(L.hpk_test_small_calls(codec._h))


class Buffers:
    """a batch's device buffers: the input `in_shift` bytes past a 16-byte boundary, the output guard | blob | guard
    with the blob `out_shift` bytes past one, out_len and status prefilled with values no kernel writes"""

    def __init__(self, b, in_shift=0, out_shift=0, fill_input=True):
        n = len(b.in_off) - 1
        src = np.zeros(in_shift + b.in_cap, np.uint8)
        if fill_input:
            src[in_shift:] = b.blob
        self.inp = to_dev(src)[in_shift:]
        self.lead = GUARD + out_shift
        self.cap = b.out_cap
        self.big = torch.full((self.lead + self.cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.out = self.big[self.lead : self.lead + self.cap]
        self.io, self.oo = off_dev(b.in_off), off_dev(b.out_off)
        self.ol = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        self.st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")

    def call(self, codec, sync=True):
        codec.decode_into(self.inp, self.io, self.out, self.oo, self.ol, self.st, device=True, sync=sync)

    def result(self):
        g = self.big.cpu().numpy()
        assert (g[: self.lead] == FILL).all(), "bytes before the output blob changed"
        assert (g[self.lead + self.cap :] == FILL).all(), "bytes behind the output blob changed"
        return g[self.lead : self.lead + self.cap], self.ol.cpu().numpy().astype(np.int64), self.st.cpu().numpy()


def decode(codec, L, b, answered, in_shift=0, out_shift=0):
    """one synchronous call; `answered`: whether the persistent kernel has to answer it"""
    buf = Buffers(b, in_shift, out_shift)
    before = small_calls(L, codec)
    buf.call(codec)
    assert small_calls(L, codec) - before == int(answered), "answered by the wrong path"
    return buf.result()


def launch_path(codec, L, b, in_shift=0, out_shift=0):
    codec.set_small_mode(0)
    try:
        return decode(codec, L, b, False, in_shift, out_shift)
    finally:
        codec.set_small_mode(*MODE)


def gap_mask(b):
    m = np.zeros(b.out_cap, bool)
    for i in np.nonzero(np.diff(b.in_off) == 0)[0]:
        m[int(b.out_off[i]) : int(b.out_off[i + 1])] = True
    return m


def assert_same(got, want_out, want_len, want_st, b, what):
    out, ol, st = got
    bad = np.nonzero(st != want_st)[0]
    assert bad.size == 0, f"{what}: status differs at {bad[:10]}: {st[bad[:10]]} for {want_st[bad[:10]]}"
    bad = np.nonzero(ol != want_len)[0]
    assert bad.size == 0, f"{what}: out_len differs at {bad[:10]}: {ol[bad[:10]]} for {want_len[bad[:10]]}"
    a, w = pc.valid_bytes(out, b.out_off, want_len), pc.valid_bytes(want_out, b.out_off, want_len)
    if not np.array_equal(a, w):
        first = int(np.nonzero(a != w)[0][0])
        lit = int(np.searchsorted(np.cumsum(want_len), first, side="right"))
        raise AssertionError(f"{what}: decoded bytes differ, first in literal {lit} of {len(ol)}")


def assert_oracle(got, name, what, gaps=True):
    """gaps: the canary gaps are unchanged too. The persistent kernel stores a literal's decoded bytes and nothing
    else, so with the mode on they must be. The launch path's kernels write a fill's whole output span back, and a
    gap is an empty literal's region, whose bytes past out_len = 0 hpk.h leaves unspecified: not asked of it."""
    b, x = pc.batch(name), pc.expected_of(name)
    assert_same(got, x.out, x.out_len, x.status, b, f"{what} against the oracle")
    if gaps:
        assert (got[0][gap_mask(b)] == FILL).all(), f"{what}: a canary gap between regions changed"


GOOD = pc.GOOD_NAMES + tuple(f"counts-{n}" for n in pc.count_list(pc.Geo(113, 8, 48, 256), pc.SM_WGS, pc.SM_MAX))


def test_names_follow_the_geometry():
    assert set(GOOD) | set(pc.BAD_NAMES) | {"over_max"} == set(pc.names())


@pytest.mark.parametrize("name", GOOD)
def test_named_batch(codec, L, name):
    b = pc.batch(name)
    t0 = time.perf_counter()
    got = decode(codec, L, b, True)
    t1 = time.perf_counter()
    assert_oracle(got, name, f"{name}, small-call mode")
    ref = launch_path(codec, L, b)
    assert_oracle(ref, name, f"{name}, launch path", gaps=False)
    assert_same(got, ref[0], ref[1], ref[2], b, f"{name}, small-call mode against the launch path")
    print(f"\n{name}: {len(b.in_off) - 1} literals, the small call {1e3 * (t1 - t0):.2f} ms with its buffers")


def test_over_max_goes_to_the_launch_path(codec, L):
    assert_oracle(decode(codec, L, pc.batch("over_max"), False), "over_max", "sm_max + 1 literals")


@pytest.mark.parametrize("name", ["store_plan", "in_place"])
def test_blob_bases(codec, L, name):
    b = pc.batch(name)
    for in_shift in (0, 1, 15):
        for out_shift in (0, 1, 15):
            assert_oracle(decode(codec, L, b, True, in_shift, out_shift), name, f"{name}, input +{in_shift}, output +{out_shift}")


@pytest.mark.parametrize("name", pc.BAD_NAMES)
def test_bad_offsets(codec, L, name):
    """the call fails as on the launch path and leaves the launch path's results; the very next good call is answered
    by the mode (the declined word holds the bad request's number, not the next one's)"""
    from loona_amd import _lib

    b = pc.batch(name)
    i = b.meta["literal"]
    runs = []
    for mode_on in (True, False):
        if not mode_on:
            codec.set_small_mode(0)
        try:
            buf = Buffers(b)
            before = small_calls(L, codec)
            with pytest.raises(RuntimeError, match="hpk_decode_batch"):
                buf.call(codec)
            assert small_calls(L, codec) == before, "a batch with bad offsets counted as answered by the mode"
            runs.append(buf.result())
        finally:
            if not mode_on:
                codec.set_small_mode(*MODE)
    (out, ol, st), (rout, rol, rst) = runs
    assert rst[i] == _lib.HPK_BAD_OFFSETS and rol[i] == 0
    assert np.array_equal(st, rst) and np.array_equal(ol, rol), f"{name}: status or out_len differs from the launch path's"
    ok = (rst != _lib.HPK_BAD_OFFSETS) & (rol > 0)
    starts = np.where(ok, b.out_off[:-1], 0)
    assert (starts + np.where(ok, rol, 0) <= b.out_cap).all()
    assert np.array_equal(pc.valid_bytes(out, starts, np.where(ok, rol, 0)), pc.valid_bytes(rout, starts, np.where(ok, rol, 0)))
    assert_oracle(decode(codec, L, pc.batch("counts-65"), True), "counts-65", f"the good call after {name}")


def test_input_written_just_before_the_call(codec, L):
    """the blob arrives by a device copy on the context's stream with work queued ahead of it and no synchronisation;
    the small call follows at once, and a torch kernel reads the outputs right after it"""
    name = "mixed_wave"
    b = pc.batch(name)
    buf = Buffers(b, 3, 5, fill_input=False)
    src = to_dev(b.blob)
    work = torch.ones(1 << 24, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    before = small_calls(L, codec)
    for _ in range(4):
        work = work * 1.0001 + 1.0
    buf.inp.copy_(src, non_blocking=True)
    buf.call(codec)
    copy = buf.big.clone()
    lens = buf.ol.sum()
    assert small_calls(L, codec) - before == 1
    assert_oracle(buf.result(), name, "input copied just before the call")
    assert np.array_equal(copy.cpu().numpy(), buf.big.cpu().numpy())
    assert int(lens.item()) == int(pc.expected_of(name).out_len.sum())
    assert float(work[0].item()) > 1.0


def test_async_call_with_the_mode_on(codec, L):
    """an HPK_ASYNC call takes the launch path; a small call behind it waits for it; both are correct"""
    a, s = Buffers(pc.batch("global")), Buffers(pc.batch("counts-513"))
    before = small_calls(L, codec)
    a.call(codec, sync=False)
    assert small_calls(L, codec) == before
    s.call(codec)
    assert small_calls(L, codec) == before + 1
    codec.sync()
    codec.check()
    assert_oracle(a.result(), "global", "the HPK_ASYNC call", gaps=False)
    assert_oracle(s.result(), "counts-513", "the small call behind it")


@pytest.mark.parametrize("G", [1, 16])
def test_workgroup_counts_and_limits(codec, L, G):
    geo = pc.geometry()
    limit = G * geo.threads * 64
    try:
        with pytest.raises(RuntimeError, match="hpk_ctx_set_small_mode"):
            codec.set_small_mode(limit + 1, G, pc.SM_IDLE_MS)
        codec.set_small_mode(limit, G, pc.SM_IDLE_MS)
        for n in pc.count_list(geo, G, 2 * G * geo.threads + 1):
            b = pc.counts_batch(n)
            x = pc.oracle_regions(b)
            assert_same(decode(codec, L, b, True), x.out, x.out_len, x.status, b, f"{n} literals, {G} workgroups")
    finally:
        codec.set_small_mode(*MODE)


def test_request_number_wrap(codec, L):
    """Request numbers wrap at 2^32. 0xFFFFFFFF is the kernel's exit command and 0 the declined word's value after a
    launch: neither may be issued. From 0xFFFFFFFC eight calls cross the wrap, each answered by the mode; after an
    idle exit the kernel is launched again with the base behind the wrap; then launches whose base lies right at the
    wrap. A library that issued 0xFFFFFFFF would spin in its relaunch loop until its own 10 s deadline and fail the
    call: this test needs the library with the fix, which is the one that has the hook."""
    assert hasattr(L, "hpk_test_small_set_request"), "the library lacks hpk_test_small_set_request (and the wrap fix)"
    from loona_amd import _lib

    name = "mixed_wave"
    b = pc.batch(name)

    def set_request(v):
        return L.hpk_test_small_set_request(codec._h, ctypes.c_uint32(v))

    try:
        codec.set_small_mode(pc.SM_MAX, pc.SM_WGS, 2)  # (2 ms idle)
        assert set_request(0xFFFFFFFF) == _lib.HPK_E_INVAL
        assert set_request(0xFFFFFFFC) == _lib.HPK_E_OK
        t0 = time.perf_counter()
        for k in range(8):  # issues 0xFFFFFFFD, 0xFFFFFFFE, 1, 2, ...
            assert_oracle(decode(codec, L, b, True), name, f"call {k} from request 0xFFFFFFFC")
        assert time.perf_counter() - t0 < 8.0, "a call ran into the library's deadline"
        time.sleep(0.05)  # the kernel has exited
        for k in range(2):
            assert_oracle(decode(codec, L, b, True), name, f"call {k} after the idle exit behind the wrap")
        for v in (0xFFFFFFFD, 0xFFFFFFFE, 0):  # the launch's base at the wrap: the next number is 0xFFFFFFFE, 1, 1
            assert set_request(v) == _lib.HPK_E_OK
            for k in range(2):
                assert_oracle(decode(codec, L, b, True), name, f"call {k} from request {v:#x}")
    finally:
        codec.set_small_mode(*MODE)
