"""GPU parity of the lane loop's round of nested body steps (lit12_round, decode v41) through the C ABI against the
library's own CPU batch path (hpk_decode_batch_cpu): out_len, status and the bytes below out_len equal, exactly,
with the wave kernel forced, in the region form (fixed chunks below 4M literals, the guided hand-out above) and
in the compacted form, sentinel bytes around the output unchanged.

In a round a lane's four body steps are nested, and a step whose second lookup holds no code (a code longer than
13 bits, or EOS) parks the lane: its leading-ones lookup runs once behind the round, for every parked lane of the
wave together. The literals here put parked and unparked lanes into the same rounds (one batch interleaves all
kinds, and a fill sorts by length only):
  lengths     text of 3..32 symbols, so that bodies end after every number of steps of a round;
  long codes  every code longer than 13 bits, and EOS, behind 0..7 seven-bit codes (one lookup each: the first and
              the second lookup of each of a round's four steps), followed by 0..4 symbols, or cut by the literal's
              end after >= 18 bits; two long codes a few lookups apart; a short and a long code of >= 31 bits
              together that end the literal exactly;
  the rest    random bytes (padding errors, EOS, long codes anywhere).
Batches: 1, 2, 63, 64, 65, 127 and 128 literals (one fill), 129 (two fills); 33,000, the least batch whose workgroup
ranges pass 128 literals, so that a wave's fill takes a whole 96-literal chunk and lanes hold two literals: the
first one's last body step is then often a parked one, in the round behind which the second literal starts; and
4M + 129 (the 33,000 tiled), the guided hand-out."""

import numpy as np
import pytest

from hpk_util import load, pack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT = 0xAB
GUARD = 256
TEXT = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789-_=;,/.:ABC ", np.uint8)


def _bits_to_bytes(v, nbits):
    """nbits bits (the integer v) as bytes, padded with ones to a byte boundary (RFC 7541 5.2)."""
    pad = (-nbits) % 8
    return ((v << pad) | ((1 << pad) - 1)).to_bytes((nbits + pad) // 8, "big") if nbits else b""


def _make_literals(n, seed):
    table = load("huffman_table.json")["table"]  # [code, len] per symbol, EOS last
    rng = np.random.default_rng(seed)
    seven = [s for s in range(256) if table[s][1] == 7]
    longs = [s for s in range(257) if table[s][1] > 13]  # EOS among them
    short = {a: [s for s in range(256) if table[s][1] == a] for a in range(5, 14)}

    def enc(syms, v=0, nb=0):
        for c in syms:
            code, ln = table[int(c)]
            v = (v << ln) | code
            nb += ln
        return v, nb

    def sevens(p):
        return [seven[int(x)] for x in rng.integers(0, len(seven), p)]

    def fits(j):  # a long code behind p one-code lookups, then 0..4 symbols
        p, s = j % 8, longs[(j // 8) % len(longs)]
        return _bits_to_bytes(*enc(sevens(p) + [s] + list(rng.choice(TEXT, (j // 3) % 5))))

    lits = []
    for i in range(n):
        k, j = i % 8, i // 8
        if k == 0:
            lits.append(_bits_to_bytes(*enc(rng.choice(TEXT, 3 + j % 30))))
        elif k == 1:
            lits.append(fits(j))
        elif k == 2:  # a long code cut by the literal's end after r >= 18 bits (whole bytes)
            p, s = j % 8, longs[(j // 8) % len(longs)]
            code, ln = table[s]
            rs = [r for r in range(18, ln) if (7 * p + r) % 8 == 0]
            if rs:
                r = rs[j % len(rs)]
                v, nb = enc(sevens(p))
                lits.append(_bits_to_bytes((v << r) | (code >> (ln - r)), nb + r))
            else:
                lits.append(fits(j))
        elif k == 3:  # two long codes 0..2 lookups apart
            a, b = longs[j % (len(longs) - 1)], longs[(j * 7) % (len(longs) - 1)]
            lits.append(_bits_to_bytes(*enc(sevens(j % 6) + [a] + sevens(j % 3) + [b] + list(rng.choice(TEXT, 3)))))
        elif k == 4:  # a short and a long code that end the literal exactly
            for _ in range(64):
                a = int(rng.integers(5, 14))
                s = longs[int(rng.integers(0, len(longs) - 1))]
                if short[a] and a + table[s][1] >= 31 and (14 * (j % 4) + a + table[s][1]) % 8 == 0:
                    lits.append(_bits_to_bytes(*enc(sevens(2 * (j % 4)) + [short[a][j % len(short[a])], s])))
                    break
            else:
                lits.append(fits(j))
        elif k == 5:
            lits.append(_bits_to_bytes(*enc(rng.choice(TEXT, int(rng.integers(8, 41))))))
        elif k == 6:  # a long code as a literal's last body step: few bits behind it
            s = longs[-1] if j % 5 == 0 else longs[j % (len(longs) - 1)]  # (every fifth: EOS)
            lits.append(_bits_to_bytes(*enc(sevens(2 + j % 7) + [s] + sevens(j % 3))))
        else:
            lits.append(rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes())
    return lits


def _cpu(blob, in_off, oo):
    """hpk_decode_batch_cpu on the caller's regions: (out_blob, out_off, out_len, status)."""
    from loona_amd import _lib

    n = len(in_off) - 1
    in_off = np.ascontiguousarray(in_off, np.uint32)
    oo = np.ascontiguousarray(oo, np.uint32)
    out = np.zeros(max(int(oo[-1]), 1), np.uint8)
    ol = np.zeros(max(n, 1), np.uint32)
    st = np.zeros(max(n, 1), np.uint8)
    rc = _lib.lib().hpk_decode_batch_cpu(blob.ctypes.data, in_off.ctypes.data, n, out.ctypes.data, oo.ctypes.data,
                                         ol.ctypes.data, st.ctypes.data, 4)
    assert rc == 0
    return out, oo, ol[:n], st[:n]


BIG = 33000
_cache = {}


def _batch(n):
    """(blob, in_off, out_off of the decoded bounds, the CPU path's result) of the first n of the BIG literals, made once."""
    if "lits" not in _cache:
        _cache["lits"] = _make_literals(BIG, 4100)
    if n not in _cache:
        blob, off = pack(_cache["lits"][:n])
        oo = np.zeros(n + 1, np.int64)
        np.cumsum((np.diff(off.astype(np.int64)) * 8) // 5, out=oo[1:])
        want = _cpu(blob, off, oo)
        if n == BIG:
            assert {0, 1, 2, 3} <= {int(s) for s in want[3]}, "the mix holds OK, both padding errors and EOS"
        _cache[n] = (blob, off, oo, want)
    return _cache[n]


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


def _valid(out, starts, ln):
    """The bytes below out_len of every literal, end to end (the same gather on numpy arrays and on torch tensors)."""
    xp = torch if isinstance(out, torch.Tensor) else np
    tot = int(ln.sum())
    ends = xp.cumsum(ln, 0)
    idx = xp.repeat_interleave(starts - (ends - ln), ln) if xp is torch else np.repeat(starts - (ends - ln), ln)
    return out[idx + (torch.arange(tot, device=out.device) if xp is torch else np.arange(tot))]


def _same(got, want, what):
    go, goo, gl, gs = got
    wo, woo, wl, ws = want
    n = len(wl)
    bad = np.nonzero(gs != ws)[0]
    assert bad.size == 0, f"{what}: status differs at {bad[:8]}: {gs[bad[:8]]} vs {ws[bad[:8]]}"
    bad = np.nonzero(gl != wl)[0]
    assert bad.size == 0, f"{what}: out_len differs at {bad[:8]}: {gl[bad[:8]]} vs {wl[bad[:8]]}"
    ln = wl.astype(np.int64)
    a, b = _valid(go, goo[:n].astype(np.int64), ln), _valid(wo, woo[:n].astype(np.int64), ln)
    if not np.array_equal(a, b):
        first = int(np.nonzero(a != b)[0][0])
        raise AssertionError(f"{what}: bytes differ, first in literal {int(np.searchsorted(np.cumsum(ln), first, side='right'))}")


SIZES = [1, 2, 63, 64, 65, 127, 128, 129, BIG]


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("n", SIZES)
def test_round_region_form(codec, n, shift):
    """Decoded-bound regions back to back (a stray byte lands in a neighbour, which is compared too) on an output
    base at +0 and +3, sentinel bytes before and past the blob."""
    blob, off, oo, want = _batch(n)
    span = int(oo[-1])
    big = torch.full((GUARD + shift + span + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    out = big[GUARD + shift : GUARD + shift + span + 1]
    ol = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    codec.decode_into(_dev(blob), _dev(off.astype(np.int32)), out, _dev(oo.astype(np.int32)), ol, st, device=True, sync=True)
    g = big.cpu().numpy()
    got = (g[GUARD + shift : GUARD + shift + span], oo, ol.cpu().numpy().astype(np.uint32), st.cpu().numpy())
    _same(got, want, f"region form, {n} literals, base +{shift}")
    assert (g[: GUARD + shift] == SENT).all(), "bytes written before the output"
    assert (g[GUARD + shift + span :] == SENT).all(), "bytes written past the output"


@pytest.mark.parametrize("n", SIZES)
def test_round_compact_form(codec, n):
    """hpk_decode_batch_compact: every literal's bytes, length and status; nothing outside [0, out_off[n])."""
    from loona_amd.batch import compact_capacity

    blob, off, _, want = _batch(n)
    need = compact_capacity(int(blob.size), n)
    big = torch.full((GUARD + need + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    _, oo, ol, st = codec.decode_compact(_dev(blob), _dev(off.astype(np.int32)), out_blob=big[GUARD : GUARD + need], sync=True)
    g = big.cpu().numpy()
    o = oo.cpu().numpy().astype(np.uint32)
    end = int(o[n])
    assert end <= need
    got = (g[GUARD : GUARD + need], o, ol[:n].cpu().numpy().astype(np.uint32), st[:n].cpu().numpy())
    _same(got, want, f"compacted form, {n} literals")
    assert (g[:GUARD] == SENT).all(), "bytes written before the output"
    assert (g[GUARD + end :] == SENT).all(), "bytes written past the reported span"
    ln = got[2].astype(np.int64)
    s = o[:n].astype(np.int64)[ln > 0]
    e = s + ln[ln > 0]
    order = np.argsort(s)
    assert (s[order][1:] >= e[order][:-1]).all(), "compacted literals overlap"


def test_round_guided_hand_out(codec):
    """4M + 129 literals, the 33,000 tiled: the guided hand-out (chunks of 1/32 of what is left, many fills a wave), region
    and compacted form. A literal's result does not depend on its place, so the expected lengths, statuses and bytes
    are the CPU path's for the 33,000, tiled; compared on the device."""
    from loona_amd.batch import compact_capacity

    blob, off, oo, want = _batch(BIG)
    n = 4_000_129
    reps, rest = divmod(n, BIG)
    off64, oo64 = off.astype(np.int64), oo.astype(np.int64)
    in_off = np.concatenate([off64[:-1] + t * off64[-1] for t in range(reps)] + [off64[: rest + 1] + reps * off64[-1]])
    out_off = np.concatenate([oo64[:-1] + t * oo64[-1] for t in range(reps)] + [oo64[: rest + 1] + reps * oo64[-1]])
    assert len(in_off) == n + 1 and in_off[-1] < 2**31 and out_off[-1] < 2**31
    src = _dev(np.concatenate([np.tile(blob, reps), blob[: int(off64[rest])]]))
    wl = np.concatenate([np.tile(want[2], reps), want[2][:rest]])
    ws = np.concatenate([np.tile(want[3], reps), want[3][:rest]])
    one = _valid(want[0], oo64[:BIG], want[2].astype(np.int64))  # a tile's valid bytes, end to end
    wb = _dev(np.concatenate([np.tile(one, reps), one[: int(want[2][:rest].sum())]]))
    ln_d, st_d = _dev(wl.astype(np.int64)), _dev(ws)
    d_in = _dev(in_off.astype(np.int32))

    def check(out, starts, ol, st, what):
        assert torch.equal(st[:n], st_d), f"{what}: status differs"
        assert torch.equal(ol[:n].to(torch.int64), ln_d), f"{what}: out_len differs"
        assert torch.equal(_valid(out, starts, ln_d), wb), f"{what}: bytes differ"

    span = int(out_off[-1])
    big = torch.full((GUARD + span + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    ol = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    st = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    d_oo = _dev(out_off.astype(np.int32))
    codec.decode_into(src, d_in, big[GUARD : GUARD + span + 1], d_oo, ol, st, device=True, sync=True)
    check(big[GUARD : GUARD + span], d_oo[:n].to(torch.int64), ol, st, "region form, 4M + 129 literals")
    assert bool((big[:GUARD] == SENT).all()) and bool((big[GUARD + span :] == SENT).all()), "bytes written outside the output"
    del big
    need = compact_capacity(int(src.numel()), n)
    big = torch.full((GUARD + need + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    _, co, ol, st = codec.decode_compact(src, d_in, out_blob=big[GUARD : GUARD + need], sync=True)
    end = int(co[n].item())
    assert end <= need
    check(big[GUARD : GUARD + need], co[:n].to(torch.int64), ol, st, "compacted form, 4M + 129 literals")
    assert bool((big[:GUARD] == SENT).all()) and bool((big[GUARD + end :] == SENT).all()), "bytes written outside the span"
