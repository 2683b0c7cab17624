"""GPU parity of the wave kernel on its 13-bit two-symbol table (decode v39) through the C ABI vs the oracle.

The wave kernel (forced) stages the 13-bit table, takes body steps while >= 31 bits are left, then the masked
tails; its waves share ONE 256-byte dummy-slot area, and a wave's window and image are 3,008 and 5,040 bytes.
Region form and compacted form; bytes, lengths and statuses against the oracle:
  a. ~4k literals of the classes the 13-bit walk can get wrong (code bits sweeping 24..48 over the body-min
     boundary, literals made only of the 13-bit pairs 6+7, 7+6, 5+8, 8+5 and only of the six 13-bit codes,
     every code of >= 13 bits as the last one, text) plus the 3,000 committed error vectors, in exact-bound
     regions back to back on an unaligned base with guard bytes: a stray byte of a tail or of the shared
     dummy area lands in a neighbour or in the guards;
  b. ~600 literals in runs of 60 (a workgroup's range): runs of 60-63 encoded bytes, whose fill the 3,008-byte
     window cuts, and runs of 20-24 encoded bytes in 88-byte regions, whose fill the 5,040-byte image cuts;
     then literals of window size - 1, window size and window size + 1;
  c. 300 literals of 64 B - 4 KiB and one of 16 KiB: the long and the huge phase read the 13-bit table;
  d. bad offsets in the middle of (a): HPK_BAD_OFFSETS, every other literal as the oracle's, guards unchanged."""

import numpy as np
import pytest

from hpk_util import compare_batches, load, oracle_decode_batch, pack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT = 0xAB
GUARD = 256
WINDOW = 3008  # hpk_decode.hip: HPK_WAVE_WIN


def _bits_to_bytes(v, nbits):
    """nbits bits (the integer v) as bytes, padded with ones to a byte boundary (RFC 7541 5.2)."""
    pad = (-nbits) % 8
    return ((v << pad) | ((1 << pad) - 1)).to_bytes((nbits + pad) // 8, "big") if nbits else b""


class _Code:
    def __init__(self):
        self.table = load("huffman_table.json")["table"]  # [code, len] per symbol, EOS last
        self.by_len = {}
        for s in range(256):
            self.by_len.setdefault(self.table[s][1], []).append(s)

    def enc(self, syms):
        v, nb = 0, 0
        for c in syms:
            code, ln = self.table[int(c)]
            v = (v << ln) | code
            nb += ln
        return _bits_to_bytes(v, nb)

    def of_bits(self, rng, bits):
        """symbols whose codes take exactly `bits` bits: mostly 5..8-bit codes, now and then any length"""
        while True:
            s, got = [], 0
            while got < bits:
                ln = int(rng.integers(5, 9)) if rng.random() < 0.94 else int(rng.integers(5, 31))
                if ln not in self.by_len or got + ln > bits:
                    if bits - got < 5:
                        break
                    continue
                s.append(int(rng.choice(self.by_len[ln])))
                got += ln
            if got == bits:
                return s


def _class_literals(rng):
    c = _Code()
    text = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789-_=;,/.:ABC ", np.uint8)
    pairs = [(6, 7), (7, 6), (5, 8), (8, 5)]
    thirteen = c.by_len[13]
    assert sorted(thirteen) == sorted([0, ord("$"), ord("@"), ord("["), ord("]"), ord("~")])
    longs = [s for s in range(256) if c.table[s][1] >= 13]
    lits = []
    for bits in range(24, 49):  # the body-min boundary (29 / 31) and a second step's
        for _ in range(60):
            lits.append(c.enc(c.of_bits(rng, bits)))
    for i in range(900):  # only 13-bit pairs / only 13-bit codes / both
        s = []
        for _ in range(int(rng.integers(1, 19))):
            if i % 3 == 0 or (i % 3 == 2 and rng.random() < 0.5):
                a, b = pairs[int(rng.integers(0, 4))]
                s += [int(rng.choice(c.by_len[a])), int(rng.choice(c.by_len[b]))]
            else:
                s.append(int(rng.choice(thirteen)))
        lits.append(c.enc(s))
    for s in longs:  # every code of >= 13 bits as the last one, behind 0..5 text bytes (every tail offset class)
        for k in range(6):
            lits.append(c.enc(list(rng.choice(text, k)) + [s]))
    for _ in range(600):  # text
        lits.append(c.enc(rng.choice(text, int(rng.integers(0, 39)))))
    return lits


_cache = {}


def _batch(kind):
    """(blob, off, the oracle's result), made once per kind and shared (never modified)."""
    if kind in _cache:
        return _cache[kind]
    rng = np.random.default_rng(1300 + len(kind))
    c = _Code()
    text = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789-_=;,/.:ABC ", np.uint8)
    tlen = np.array([c.table[s][1] for s in range(256)], np.int64)

    def of_bytes(lo, hi):  # text whose encoding has lo..hi bytes (its codes are <= 8 bits: no byte is skipped)
        want = int(rng.integers(lo, hi + 1))
        s = rng.choice(text, want * 8 // 5 + 2)
        bits = np.cumsum(tlen[s])
        e = c.enc(s[: int(np.searchsorted(bits, 8 * want - 8, side="right")) + 1])  # the first count past 8 want - 8 bits
        assert len(e) == want
        return e

    if kind == "classes":
        lits = _class_literals(rng)
        lits += [bytes.fromhex(v["in"]) for v in load("error_vectors.json")["vectors"]]
        order = rng.permutation(len(lits))
        lits = [lits[i] for i in order]
    elif kind == "cuts":
        lits = []
        for run in range(10):
            lits += [of_bytes(60, 63) if run % 2 else of_bytes(20, 24) for _ in range(60)]
        lits += [of_bytes(WINDOW - 1, WINDOW - 1), of_bytes(WINDOW, WINDOW), of_bytes(WINDOW + 1, WINDOW + 1)]
    else:  # "long"
        lits = []
        for i in range(300):
            nb = int(rng.integers(64, 4097))
            lits.append(of_bytes(nb - 8, nb) if i % 4 else rng.integers(0, 256, nb, dtype=np.uint8).tobytes())
        lits.insert(150, of_bytes(16384 - 16, 16384))
    blob, off = pack(lits)
    _cache[kind] = (blob, off, oracle_decode_batch(blob, off))
    return _cache[kind]


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU)")
    from loona_amd import HuffmanCodec

    c = HuffmanCodec(0, stream=torch.cuda.current_stream())
    c.set_decode_kernel("wave")
    yield c
    c.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _regions(kind, off):
    """out_off: exact-bound regions back to back; "cuts": the 20-24-byte runs in 88-byte regions"""
    bound = (np.diff(off.astype(np.int64)) * 8) // 5
    if kind == "cuts":
        nb = np.diff(off.astype(np.int64))
        bound = np.where(nb <= 24, 88, bound)
    oo = np.zeros(len(off), np.int64)
    np.cumsum(bound, out=oo[1:])
    return oo


def _decode_regions(codec, blob, off_dev, oo, shift, sync=True):
    n = len(oo) - 1
    big = torch.full((GUARD + shift + int(oo[-1]) + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    out = big[GUARD + shift : GUARD + shift + int(oo[-1]) + 1]
    ol = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    err = None
    try:
        codec.decode_into(_dev(blob), off_dev, out, _dev(oo.astype(np.int32)), ol, st, device=True, sync=sync)
    except RuntimeError as e:
        err = e
    g = big.cpu().numpy()
    assert (g[: GUARD + shift] == SENT).all(), "bytes written before the output"
    assert (g[GUARD + shift + int(oo[-1]) :] == SENT).all(), "bytes written past the output"
    return g[GUARD + shift : GUARD + shift + int(oo[-1])], ol.cpu().numpy().astype(np.uint32), st.cpu().numpy(), err


@pytest.mark.parametrize("kind,shift", [("classes", 3), ("classes", 0), ("cuts", 5), ("long", 3)])
def test_lut13_region_form(codec, kind, shift):
    blob, off, ref = _batch(kind)
    oo = _regions(kind, off)
    outn, ol, st, err = _decode_regions(codec, blob, _dev(off.astype(np.int32)), oo, shift)
    assert err is None, err
    if kind == "classes":
        assert len({int(s) for s in ref[3]}) == 4, "the mix holds OK, both padding errors and EOS"
    compare_batches((outn, oo.astype(np.uint32), ol, st), ref, f"13-bit table, region form, {kind}, base +{shift}")


@pytest.mark.parametrize("kind", ["classes", "cuts", "long"])
def test_lut13_compact_form(codec, kind):
    """hpk_decode_batch_compact: every literal's bytes, length and status; nothing outside [0, out_off[n])."""
    from loona_amd.batch import compact_capacity

    blob, off, ref = _batch(kind)
    n = len(off) - 1
    need = compact_capacity(int(blob.size), n)
    big = torch.full((GUARD + need + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    out, oo, ol, st = codec.decode_compact(_dev(blob), _dev(off.astype(np.int32)), out_blob=big[GUARD : GUARD + need], sync=True)
    g = big.cpu().numpy()
    o = oo.cpu().numpy().astype(np.uint32)
    end = int(o[n])
    assert end <= need
    got = (g[GUARD : GUARD + need], o, ol[:n].cpu().numpy().astype(np.uint32), st[:n].cpu().numpy())
    compare_batches(got, ref, f"13-bit table, compacted form, {kind}")
    assert (g[:GUARD] == SENT).all(), "bytes written before the output"
    assert (g[GUARD + end :] == SENT).all(), "bytes written past the reported span"
    ln = got[2].astype(np.int64)
    s = o[:n].astype(np.int64)[ln > 0]
    e = s + ln[ln > 0]
    order = np.argsort(s)
    assert (s[order][1:] >= e[order][:-1]).all(), "compacted literals overlap"


def test_lut13_bad_offsets_in_the_middle(codec):
    """A decreasing offset in the middle of (a): that literal's workgroup range gets HPK_BAD_OFFSETS from there
    (out_len 0), the synchronous call raises, every literal not marked decodes as the oracle's (but the one
    before the bad offset, whose end moved), and the guard bytes stay."""
    from loona_amd import _lib

    blob, off, ref = _batch("classes")
    n = len(off) - 1
    oo = _regions("classes", off)
    io = off.astype(np.int64).copy()
    j = n // 2 + 7
    io[j] = io[j + 1] + 3
    outn, ol, st, err = _decode_regions(codec, blob, _dev(io.astype(np.uint32).view(np.int32)), oo, 3)
    assert err is not None and "hpk_decode_batch" in str(err)
    bad = st == _lib.HPK_BAD_OFFSETS
    assert bad[j] and (ol[bad] == 0).all()
    good = ~bad
    good[j - 1] = False
    assert good.sum() > n // 2
    assert np.array_equal(st[good], ref[3][good]) and np.array_equal(ol[good], ref[2][good])
    idx = np.nonzero(good)[0]
    sel = lambda o, oof: np.concatenate([o[int(oof[i]) : int(oof[i]) + int(ref[2][i])] for i in idx])  # noqa: E731
    assert np.array_equal(sel(outn, oo), sel(ref[0], ref[1])), "a literal outside the bad range decoded differently"
    # the same buffers with good offsets decode normally afterwards
    outn, ol, st, err = _decode_regions(codec, blob, _dev(off.astype(np.int32)), oo, 3)
    assert err is None
    compare_batches((outn, oo.astype(np.uint32), ol, st), ref, "after the bad offsets")
