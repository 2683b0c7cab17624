"""GPU parity of the host-pointer batches (hpk_decode_batch / hpk_encode_batch with HPK_PTR_HOST) through their
chunked pipeline, against the C oracle, bit for bit.

Every placed case of tests/host_chunk_cases.py (test_host_chunk_cases.py proves on the CPU that each reaches the
cut it is named for) goes through the C ABI itself with the fill and the wave kernel forced, from pageable
buffers and again with both blobs page-locked (hpk_host_register). A run compares status, out_len and each
literal's first out_len bytes with the oracle's answer, and then what the call must not have touched: the bytes of
out_blob before out_off[0] and behind out_off[n], the entries of out_len and status behind index n, in_blob and
both offset arrays. Around them: a differential batch of 60,000 literals with errors and short regions, decoded
and encoded back; calls the library refuses (HPK_E_INVAL) and what they leave behind; one context used for small
and chunked host calls and device calls in turn, with and without the small-call mode; four contexts on four
threads at once; and the block decoder's trusted form of the same pipeline (hpack.decode_blocks with a ctx) on
blocks built by hand around the model's cuts.

The buffers are tens of MiB (mostly declared capacity). Measured on an MI355X: the whole file (93 tests) in 7.3 s;
the longest test is test_differential_decode[fill] at 1.7 s (it builds the batch and asks the oracle; the wave run
that reuses both takes 0.09 s), then test_one_context_over_time at 0.4 s; a placed case takes about 0.05 s."""

import functools
import threading

import numpy as np
import pytest

import host_chunk_cases as hc
from decode_long_cases import LEN, gather
from hpk_util import oracle_decode_batch, oracle_encode, oracle_encode_batch, pack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CANARY, LEN_CANARY, ST_CANARY, TAIL = 0xA5, 0xDEADBEEF, 0xEE, 64
_LEN = np.array(LEN[:256], np.int64)
MC = hc.MAX_CHUNKS


def _codec(stream="own", kernel="auto"):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU)")
    from loona_amd import HuffmanCodec

    c = HuffmanCodec(0, stream=stream)
    c.set_decode_kernel(kernel)
    return c


@pytest.fixture(scope="module", params=["fill", "wave"])
def codec(request):
    c = _codec(kernel=request.param)
    yield c
    c.close()


@pytest.fixture(scope="module")
def plain():
    c = _codec()
    yield c
    c.close()


def _own_pages(nbytes, fill):
    """nbytes on pages that nothing else shares (page-locking goes by pages: two small blobs of one page could not
    both be registered)"""
    raw = np.empty(nbytes + 8192, np.uint8)
    at = -raw.ctypes.data % 4096
    a = raw[at : at + nbytes]
    a[:] = fill
    return a


class Run:
    """The caller's side of one host call: the arrays it passes, canaries where the call must not write, and
    copies of what it must not change."""

    def __init__(self, c):
        self.case, self.n = c, len(c.lits)
        self.in_blob = _own_pages(max(c.in_cap, 1), 0)
        self.in_blob[:] = hc.in_blob(c)
        self.in_off, self.out_off = c.in_off.astype(np.uint32), c.out_off.astype(np.uint32)
        self.keep = (self.in_blob.copy(), self.in_off.copy(), self.out_off.copy())
        self.out_blob = _own_pages(c.out_cap + TAIL, CANARY)
        self.out_len = np.full(self.n + 8, LEN_CANARY, np.uint32)
        self.status = np.full(self.n + 8, ST_CANARY, np.uint8)

    def call(self, h, registered=False, **over):
        """the C call; over: arguments replaced (in_blob, in_cap, in_off, n, out_blob, out_cap, out_off, out_len, status)"""
        from loona_amd import _lib

        L, c = _lib.lib(), self.case
        a = dict(in_blob=self.in_blob.ctypes.data, in_cap=c.in_cap, in_off=self.in_off.ctypes.data, n=self.n,
                 out_blob=self.out_blob.ctypes.data, out_cap=c.out_cap, out_off=self.out_off.ctypes.data,
                 out_len=self.out_len.ctypes.data, status=self.status.ctypes.data)
        a.update(over)
        fn = L.hpk_decode_batch if c.kind == "decode" else L.hpk_encode_batch
        pinned = [self.in_blob, self.out_blob] if registered else []
        for x in pinned:
            assert L.hpk_host_register(x.ctypes.data, x.nbytes) == 0
        try:
            return fn(h, a["in_blob"], a["in_cap"], a["in_off"], a["n"], a["out_blob"], a["out_cap"], a["out_off"],
                      a["out_len"], a["status"], _lib.HPK_PTR_HOST)
        finally:
            for x in pinned:
                assert L.hpk_host_unregister(x.ctypes.data) == 0

    def untouched_inputs(self, what):
        for got, kept, name in zip((self.in_blob, self.in_off, self.out_off), self.keep, ("in_blob", "in_off", "out_off")):
            assert np.array_equal(got, kept), f"{what}: the call changed {name}"

    def all_canary(self, what):
        assert (self.out_blob == CANARY).all(), f"{what}: out_blob written"
        assert (self.out_len == LEN_CANARY).all() and (self.status == ST_CANARY).all(), f"{what}: out_len / status written"
        self.untouched_inputs(what)

    def check(self, ex, what):
        n, c = self.n, self.case
        bad = np.nonzero(self.status[:n] != ex.status)[0]
        assert bad.size == 0, f"{what}: status differs at {bad[:8]} ({self.status[bad[:8]]} vs {ex.status[bad[:8]]})"
        bad = np.nonzero(self.out_len[:n] != ex.out_len)[0]
        assert bad.size == 0, f"{what}: out_len differs at {bad[:8]} ({self.out_len[bad[:8]]} vs {ex.out_len[bad[:8]]})"
        got = gather(self.out_blob, c.out_off, ex.out_len)
        if not np.array_equal(got, ex.flat):
            first = int(np.nonzero(got != ex.flat)[0][0])
            lit = int(np.searchsorted(np.cumsum(ex.out_len), first, side="right"))
            raise AssertionError(f"{what}: bytes differ (first at byte {first} of the results, literal {lit})")
        lo, hi = int(c.out_off[0]), int(c.out_off[-1])
        assert (self.out_blob[:lo] == CANARY).all(), f"{what}: bytes before out_off[0] written"
        assert (self.out_blob[hi:] == CANARY).all(), f"{what}: bytes behind out_off[n] written"
        assert (self.out_len[n:] == LEN_CANARY).all() and (self.status[n:] == ST_CANARY).all(), \
            f"{what}: out_len / status written behind index n"
        self.untouched_inputs(what)


def run_case(h, c, ex, what, registered=False):
    r = Run(c)
    rc = r.call(h, registered)
    assert rc == 0, f"{what}: rc {rc}"
    r.check(ex, what)
    return r


def results(r, ex, first=0):
    """(status, out_len, bytes) of literals first .. n - 1 of a run"""
    return (r.status[first : r.n].tolist(), r.out_len[first : r.n].tolist(),
            gather(r.out_blob, r.case.out_off[first:], ex.out_len[first:]).tobytes())


# ---- the placed cases ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", hc.DECODE_NAMES)
def test_decode_case(codec, name):
    c, ex = hc.case(name), hc.expected_of(name)
    for registered in (False, True):
        run_case(codec._h, c, ex, f"{name} ({'page-locked' if registered else 'pageable'})", registered)


@pytest.mark.parametrize("name", hc.ENCODE_NAMES)
def test_encode_case(plain, name):
    c, ex = hc.case(name), hc.expected_of(name)
    for registered in (False, True):
        run_case(plain._h, c, ex, f"{name} ({'page-locked' if registered else 'pageable'})", registered)


def test_cut_alignment_gives_identical_results(codec):
    """the same literals with every cut at 0, 1 and 15 mod 16 of the input: a kernel's 16-byte load across a cut
    reaches into bytes whose copy may still be in flight; the literals' results must not depend on it"""
    seen = []
    for shift in (0, 1, 15):
        for registered in (False, True):
            name = f"align-{shift}"
            seen.append(results(run_case(codec._h, hc.case(name), hc.expected_of(name), name, registered),
                                hc.expected_of(name), first=1))
    assert all(x == seen[0] for x in seen)


# ---- the differential batch ----------------------------------------------------------------------------------------

def test_differential_decode(codec):
    c, ex = hc.differential()
    # on the oracle's answer alone, before the GPU is touched: every status occurs, and the model says 8 chunks
    assert all(int((ex.status == s).sum()) >= 10 for s in (1, 2, 3, 4)), np.bincount(ex.status)
    assert hc.cuts(c.in_off, c.out_off)[0] == MC
    run_case(codec._h, c, ex, "differential decode")


@functools.lru_cache(maxsize=1)
def _differential_encode():
    """the differential batch's valid decoded strings as an encode case: regions of the oracle's encoded length plus
    0 to 3 bytes plus a fixed pad that makes 8 chunks"""
    c, ex = hc.differential()
    ok = np.nonzero(ex.status == 0)[0]
    ends = np.cumsum(ex.out_len)
    flat = ex.flat.tobytes()
    raws = [flat[int(ends[i] - ex.out_len[i]) : int(ends[i])] for i in ok]
    _, _, ol, st = oracle_encode_batch(*pack(raws))
    assert not st.any()
    rng = np.random.default_rng(11)
    caps = ol.astype(np.int64) + rng.integers(0, 4, len(raws))
    need = MC * hc.CHUNK_BYTES - sum(len(x) for x in raws) - int(caps.sum())
    caps += max(0, -(-need // len(raws)))
    e = hc.place("encode", raws, [int(x) for x in caps])
    return e, hc.expected(e)


def test_differential_encode(plain):
    e, ex = _differential_encode()
    assert hc.cuts(e.in_off, e.out_off)[0] == MC and not ex.status.any()
    run_case(plain._h, e, ex, "differential encode")


# ---- refused calls -------------------------------------------------------------------------------------------------

def _refusals(c):
    """name -> the arguments replaced; each is refused on the host before any copy or launch"""
    n = len(c.lits)

    def off(a, i, v):
        a = a.astype(np.uint32)
        a[i] = v
        return a

    io, oo = c.in_off, c.out_off
    return {
        "in_off decreasing at 0": dict(in_off=off(io, 0, io[1] + 1)),
        "in_off decreasing in the middle": dict(in_off=off(io, n // 2, io[n // 2 - 1] - 1)),
        "in_off decreasing at n": dict(in_off=off(io, n, io[n - 1] - 1)),
        "out_off decreasing": dict(out_off=off(oo, n // 2, oo[n // 2 - 1] - 1)),
        "in_off[n] past in_cap": dict(in_cap=int(io[n]) - 1),
        "out_off[n] past out_cap": dict(out_cap=int(oo[n]) - 1),
        "null out_len": dict(out_len=None),
        "null in_blob": dict(in_blob=None),
    }


def _refused(r, h, over):
    """the call with the arguments of one refusal"""
    return r.call(h, **{k: (v.ctypes.data if isinstance(v, np.ndarray) else v) for k, v in over.items()})


@pytest.mark.parametrize("fn", ["decode", "encode"])
def test_refused_calls_leave_no_trace(plain, fn):
    """Each call is rejected by the offset and null checks on the host (HPK_E_INVAL): every output array and blob is
    still all canary, the inputs are unchanged, hpk_ctx_check is clean, and the same context answers the next
    valid call. The blobs are as large as every call claims."""
    from loona_amd import _lib

    name = "bases-decode" if fn == "decode" else "bases-encode"
    c, ex = hc.case(name), hc.expected_of(name)
    refusals = _refusals(c)
    assert len(refusals) == 8
    for what, over in refusals.items():
        r = Run(c)
        rc = _refused(r, plain._h, over)
        assert rc == _lib.HPK_E_INVAL, f"{what}: rc {rc}"
        r.all_canary(what)
        assert _lib.lib().hpk_ctx_check(plain._h) == 0, what
        run_case(plain._h, c, ex, f"the valid call after '{what}'")


def test_empty_batch_with_null_blobs(plain):
    from loona_amd import _lib

    L = _lib.lib()
    zero = np.zeros(1, np.uint32)
    for fn in (L.hpk_decode_batch, L.hpk_encode_batch):
        assert fn(plain._h, None, 0, zero.ctypes.data, 0, None, 0, zero.ctypes.data, None, None, _lib.HPK_PTR_HOST) == 0
    assert L.hpk_ctx_check(plain._h) == 0 and zero[0] == 0


# ---- one context over time -----------------------------------------------------------------------------------------

def _device_batch():
    from loona_amd import synth

    w = synth.config2(n=3000, seed=17)
    return w, oracle_decode_batch(w.enc_blob, w.enc_off)


def _device_result(r, n):
    out, oo, ol, st = r
    return out.cpu().numpy(), oo.cpu().numpy().astype(np.uint32), ol[:n].cpu().numpy().astype(np.uint32), st[:n].cpu().numpy()


@pytest.mark.parametrize("small_mode", [False, True])
def test_one_context_over_time(small_mode):
    """A small host call, the 8-chunk one, the small one again (the staging buffers grow, and keep the earlier
    call's bytes); a host call right behind an HPK_ASYNC device call on the caller's stream, and a device call
    right behind a host call. With the small-call mode on, the persistent kernel answers the synchronous device
    call and no host call."""
    from hpk_util import compare_batches

    from loona_amd import _lib

    w, want = _device_batch()
    s = torch.cuda.Stream()
    c = _codec(stream=s)
    try:
        if small_mode:
            c.set_small_mode(65536, 4, 200)
        for name in ("small3", "target-on", "small3", "seam-size-8192", "no-input", "small3"):
            run_case(c._h, hc.case(name), hc.expected_of(name), f"{name} in turn")
        dblob = torch.from_numpy(w.enc_blob).cuda()
        doff = torch.from_numpy(w.enc_off.astype(np.int32)).cuda()
        torch.cuda.synchronize()
        answered = _lib.lib().hpk_test_small_calls(c._h)
        r = c.decode_device(dblob, doff, sync=False)  # HPK_ASYNC, still running or queued when the host call starts
        run_case(c._h, hc.case("empties-on-cut"), hc.expected_of("empties-on-cut"), "host call behind an async device call")
        s.synchronize()
        compare_batches(_device_result(r, w.n), want, "async device call in front of a host call")
        run_case(c._h, hc.case("small3"), hc.expected_of("small3"), "small host call")
        r = c.decode_device(dblob, doff, sync=True)
        torch.cuda.synchronize()
        compare_batches(_device_result(r, w.n), want, "device call behind a host call")
        run_case(c._h, hc.case("bases-decode"), hc.expected_of("bases-decode"), "host call behind a device call")
        c.check()
        assert _lib.lib().hpk_test_small_calls(c._h) - answered == (1 if small_mode else 0)
    finally:
        if small_mode:
            c.set_small_mode(0)
        torch.cuda.synchronize()
        c.close()


# ---- one context per thread ----------------------------------------------------------------------------------------

def test_one_context_per_thread():
    """Four threads, each with its own context, each making five 8-chunk host decodes of its own batch at the same
    time (ctypes releases the GIL for the call), then one refused call of its own kind: every result against the
    oracle, and each thread's hpk_last_error its own."""
    from loona_amd import _lib

    L = _lib.lib()
    names = ("target-on", "empties-on-cut", "align-15", "bases-decode")
    refusal = (("in_off decreasing at 0", b"non-decreasing"), ("in_off[n] past in_cap", b"capacity"),
               ("null out_len", b"null argument"), ("null in_blob", b"null blob"))
    work = [(hc.case(n), hc.expected_of(n)) for n in names]
    codecs = [_codec() for _ in names]
    barrier = threading.Barrier(len(names))
    failed, messages = [None] * len(names), [None] * len(names)

    def thread(t):
        try:
            c, ex = work[t]
            barrier.wait(timeout=120)
            for rep in range(5):
                run_case(codecs[t]._h, c, ex, f"thread {t}, call {rep}")
            r = Run(c)
            assert _refused(r, codecs[t]._h, _refusals(c)[refusal[t][0]]) == _lib.HPK_E_INVAL
            barrier.wait(timeout=120)  # every thread has been refused: the messages are read after all were written
            messages[t] = L.hpk_last_error(codecs[t]._h)
        except BaseException as e:  # noqa: BLE001 (handed to the main thread)
            failed[t] = e
            barrier.abort()

    threads = [threading.Thread(target=thread, args=(t,)) for t in range(len(names))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    try:
        for e in failed:
            if e is not None and not isinstance(e, threading.BrokenBarrierError):
                raise e
        assert not any(failed), failed
        for t, (_, text) in enumerate(refusal):
            assert text in messages[t], (t, messages)
        assert len(set(messages)) == len(names)
    finally:
        for c in codecs:
            c.close()


# ---- the block decoder's trusted form ------------------------------------------------------------------------------

def _hp_int(value, prefix_bits, flags):
    """RFC 7541 5.1"""
    top = (1 << prefix_bits) - 1
    if value < top:
        return bytes([flags | value])
    out, value = [flags | top], value - top
    while value >= 128:
        out.append(value % 128 + 128)
        value //= 128
    return bytes(out + [value])


def _field(name, value, huffman=True, bad=False):
    """(a never-indexed literal field with a new name: the name raw, the value a Huffman string (or raw), the
    Huffman string's bytes or None). bad: a zero in the value's padding (it has at least one bit of it)."""
    v = value
    if huffman:
        v = oracle_encode(value)
        if bad:
            assert int(_LEN[np.frombuffer(value, np.uint8)].sum()) % 8
            v = v[:-1] + bytes([v[-1] & 0xFE])
    return b"\x10" + _hp_int(len(name), 7, 0) + name + _hp_int(len(v), 7, 0x80 if huffman else 0) + v, v if huffman else None


def _text(rng, n):
    """n characters of text (one more where needed) whose Huffman form ends in at least one bit of padding"""
    t = rng.choice(hc.TEXT, n).tobytes()
    if int(_LEN[np.frombuffer(t, np.uint8)].sum()) % 8 == 0:
        t += b"0"  # (a 5-bit code)
    return t


class Blocks:
    """Header blocks built from known header lists: want[b] is block b's header list, or its error; lits are the
    Huffman strings in batch order, from which the model gives the cuts of the trusted host batch (regions of the
    4-rounded decoded bound, as hpk_hdec_decode_blocks lays them out)."""

    def __init__(self):
        self.wire, self.want, self.lits, self.last_lit = [], [], [], []

    def add(self, headers, huffman=True, bad=False):
        """headers: [(name, value)]; bad: the last value's padding is invalid, the block's result is that error"""
        from loona_amd import hpack

        w = b""
        for k, (name, value) in enumerate(headers):
            f, lit = _field(name, value, huffman, bad and k == len(headers) - 1)
            w += f
            if lit is not None:
                self.lits.append(lit)
        self.wire.append(w)
        self.last_lit.append(len(self.lits) - 1 if huffman and headers else None)
        self.want.append(hpack.DecoderError("StringDecodingError", ("HuffmanDecoderError", 2)) if bad else list(headers))
        return len(self.wire) - 1

    def cuts(self):
        lens = np.array([len(x) for x in self.lits], np.int64)
        in_off = np.concatenate([[0], np.cumsum(lens)])
        out_off = np.concatenate([[0], np.cumsum((8 * lens // 5 + 3) & ~3)])
        return hc.cuts(in_off, out_off)

    def decode(self, codec):
        from loona_amd import hpack

        decs = [hpack.Decoder() for _ in self.wire]
        return hpack.decode_blocks(list(zip(decs, self.wire)), codec), [d.table_size() for d in decs]


@functools.lru_cache(maxsize=1)
def _big_value():
    return _text(np.random.default_rng(61), 8_000_000)


def _small_block(b, rng, k):
    b.add([(b"x-small-%d" % k, _text(rng, int(rng.integers(3, 40)))), (b"x-other", _text(rng, int(rng.integers(1, 20))))])


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_blocks_collapsed_cuts(codec, where):
    """one block carries a Huffman value of about 6 MiB among 50 small blocks: every cut of the trusted batch is
    that string, so the apply threads wait for empty chunks before or behind the full one"""
    rng = np.random.default_rng(62)
    b = Blocks()
    at = {"first": 0, "middle": 25, "last": 50}[where]
    for k in range(50):
        if k == at:
            big = b.add([(b"x-lead", _text(rng, 9)), (b"x-big", _big_value())])
        _small_block(b, rng, k)
    if at == 50:
        big = b.add([(b"x-lead", _text(rng, 9)), (b"x-big", _big_value())])
    chunks, cut = b.cuts()
    assert chunks >= 3 and cut[1:chunks] == [b.last_lit[big]] * (chunks - 1)
    assert len(b.lits[b.last_lit[big]]) > 6_000_000
    got, tables = b.decode(codec)
    assert got == b.want
    assert tables == [(0, 0, 4096)] * len(b.wire)


@functools.lru_cache(maxsize=4)
def _boundary_blocks(layout, bad):
    """Seven blocks of a large (about 1 MB) and a small Huffman value, the large one last ("first": it takes a cut,
    so the block's last string is the first literal of a chunk) or first ("last": the block in front ends in the
    small one, the last literal of a chunk), with a block of raw strings only between every two of them. bad: the
    blocks at the cuts have invalid padding in their last string."""
    rng = np.random.default_rng(63)
    values = [(_text(rng, 1_250_000 + 1000 * k), _text(rng, 12 + k)) for k in range(7)]

    def build(bad_blocks):
        b = Blocks()
        for k, (large, small) in enumerate(values):
            pair = [(b"x-small", small), (b"x-large", large)] if layout == "first" else [(b"x-large", large), (b"x-small", small)]
            b.add(pair, bad=2 * k in bad_blocks)  # (block 2 k: a block of raw strings follows each)
            b.add([(b"x-raw-%d" % k, b"no huffman string here")], huffman=False)
        return b

    b = build(())
    chunks, cut = b.cuts()
    assert chunks >= 4
    seams = []  # the blocks whose last string lies on a cut
    for j in range(1, chunks):
        lit = cut[j] if layout == "first" else cut[j] - 1
        assert lit in b.last_lit and cut[j] > cut[j - 1], (layout, cut)
        seams.append(b.last_lit.index(lit))
        if layout == "first":
            assert len(b.lits[lit]) > 900_000  # the large value: the block's last string opens chunk j
        else:
            assert len(b.lits[lit]) < 64 and len(b.lits[cut[j]]) > 900_000  # the small one closes chunk j - 1
    assert len(set(seams)) == chunks - 1
    if bad:
        b = build(tuple(seams))
        assert b.cuts() == (chunks, cut)
    return b, seams


@pytest.mark.parametrize("bad", [False, True])
@pytest.mark.parametrize("layout", ["first", "last"])
def test_blocks_last_string_on_a_cut(codec, layout, bad):
    """a block's last string as the first and as the last literal of a chunk, a block without a Huffman string
    behind it: the apply thread must have waited for exactly the chunks that hold the block's strings. With an
    error (invalid padding) in those last strings, the blocks at the cuts give that error and every other block its
    headers, as the host path (no ctx) does, table sizes included."""
    from loona_amd import hpack

    b, seams = _boundary_blocks(layout, bad)
    got, tables = b.decode(codec)
    for k, (g, w) in enumerate(zip(got, b.want)):
        assert g == w, f"block {k}"
    assert [k for k, g in enumerate(got) if isinstance(g, hpack.DecoderError)] == (sorted(seams) if bad else [])
    host, host_tables = b.decode(None)
    assert got == host and tables == host_tables
