"""GPU parity of the wave fills' masked tails (lit12_tail, decode v38) through the C ABI vs the oracle.

A literal's last <= 28 bits are decoded by four masked lookups with no fit test; a lane whose tail holds a
13..28-bit code or a code cut by the literal's end falls back to the checked steps. The batches here put
both kinds of lanes into the same waves: text of 8-64 bytes, literals of 1-3 encoded bytes (no body step),
5-bit-only text (the decoded length reaches the bound), literals ending in a 13..28-bit code, and bad
padding, padding of more than 7 bits and EOS as the last code (the reference's error vectors among them),
interleaved. 4,096 literals are 16 waves x 2 fills, 300 one workgroup's partial last fill. Region form
(exact-bound regions back to back) and the compacted form, under both forced kernels: every byte, length and
status equals the oracle's, the sentinel bytes around the output unchanged."""

import numpy as np
import pytest

from hpk_util import compare_batches, load, oracle_decode_batch, pack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT = 0xAB
GUARD = 256


def _bits_to_bytes(v, nbits):
    """nbits bits (the integer v) as bytes, padded with ones to a byte boundary (RFC 7541 5.2)."""
    pad = (-nbits) % 8
    return ((v << pad) | ((1 << pad) - 1)).to_bytes((nbits + pad) // 8, "big") if nbits else b""


def _make_literals(n, seed):
    table = load("huffman_table.json")["table"]  # [code, len] per symbol, EOS last

    def enc_bits(s):
        v, nb = 0, 0
        for c in s:
            code, ln = table[c]
            v = (v << ln) | code
            nb += ln
        return v, nb

    rng = np.random.default_rng(seed)
    five = np.frombuffer(b"012aceiost", np.uint8)
    text = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789-_=;,/.:ABC ", np.uint8)
    longs = [s for s in range(256) if 13 <= table[s][1] <= 28]
    vecs = [bytes.fromhex(k["in"]) for k in load("kat.json") if k["status"] != 0]
    vecs += [bytes.fromhex(v["in"]) for v in load("error_vectors.json")["vectors"] if v["status"] != 0 and len(v["in"]) <= 128]
    lits = []
    for i in range(n):
        k = i % 7
        if k == 0:  # text of 8-64 bytes
            lits.append(_bits_to_bytes(*enc_bits(rng.choice(text, int(rng.integers(8, 65))))))
        elif k == 1:  # 1-3 encoded bytes: no body step; valid text or random bits
            if rng.random() < 0.5:
                v, nb = enc_bits(rng.choice(text, int(rng.integers(1, 4))))
                lits.append(_bits_to_bytes(v, nb)[:3])
            else:
                lits.append(rng.integers(0, 256, int(rng.integers(1, 4)), dtype=np.uint8).tobytes())
        elif k == 2:  # 5-bit codes only: the decoded length reaches the region's size
            lits.append(_bits_to_bytes(*enc_bits(rng.choice(five, int(rng.integers(1, 70))))))
        elif k == 3:  # text, then a 13..28-bit code as the last one
            s = list(rng.choice(text, int(rng.integers(0, 40)))) + [int(rng.choice(longs))]
            lits.append(_bits_to_bytes(*enc_bits(s)))
        elif k == 4:  # text, then an error as the last code
            v, nb = enc_bits(rng.choice(text, int(rng.integers(0, 40))))
            kind = int(rng.integers(0, 4))
            if kind == 0:  # bad padding: the last bits hold a zero and no whole code
                b = bytearray(_bits_to_bytes((v << 4) | int(rng.integers(0, 15)), nb + 4))
                lits.append(bytes(b))
            elif kind == 1:  # padding of more than 7 bits
                lits.append(_bits_to_bytes(v, nb) + b"\xff" * int(rng.integers(1, 3)))
            elif kind == 2:  # EOS
                lits.append(_bits_to_bytes((v << 30) | ((1 << 30) - 1), nb + 30))
            else:  # a code cut by the literal's end
                code, ln = table[int(rng.choice(longs))]
                cut = int(rng.integers(1, ln))
                lits.append(_bits_to_bytes((v << cut) | (code >> (ln - cut)), nb + cut)[: (nb + cut) // 8 + 1])
        elif k == 5:  # the reference's error vectors as they are
            lits.append(vecs[(i // 7) % len(vecs)])
        else:  # random bytes
            lits.append(rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes())
    return lits


_cache = {}


def _batch(n):
    """(blob, off, the oracle's result), made once per size and shared (never modified)."""
    if n not in _cache:
        blob, off = pack(_make_literals(n, 3800 + n))
        ref = oracle_decode_batch(blob, off)
        st = ref[3]
        assert len({int(s) for s in st}) >= 4, "the mix holds OK, both padding errors and EOS"
        _cache[n] = (blob, off, ref)
    return _cache[n]


@pytest.fixture(scope="module")
def codec():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m 'not gpu' on CPU)")
    from loona_amd import HuffmanCodec

    c = HuffmanCodec(0, stream=torch.cuda.current_stream())
    yield c
    c.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("kernel", ["wave", "fill"])
@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("n", [4096, 300])
def test_masked_tails_region_form(codec, n, shift, kernel):
    """Exact-bound regions back to back (a stray byte lands in a neighbour, which is compared with the
    oracle; the C ABI's regions are contiguous, out_off[i + 1] is region i's end, so there is no room for
    sentinels between them) on an output base at +0 and +3, sentinel bytes before and past the blob."""
    blob, off, ref = _batch(n)
    codec.set_decode_kernel(kernel)
    bound = (np.diff(off.astype(np.int64)) * 8) // 5
    oo = np.zeros(n + 1, np.int64)
    np.cumsum(bound, out=oo[1:])
    big = torch.full((GUARD + shift + int(oo[-1]) + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    out = big[GUARD + shift : GUARD + shift + int(oo[-1]) + 1]
    ol = torch.zeros(n, dtype=torch.int32, device="cuda")
    st = torch.zeros(n, dtype=torch.uint8, device="cuda")
    codec.decode_into(_dev(blob), _dev(off.astype(np.int32)), out, _dev(oo.astype(np.int32)), ol, st, device=True, sync=True)
    codec.set_decode_kernel("auto")
    g = big.cpu().numpy()
    outn = g[GUARD + shift : GUARD + shift + int(oo[-1])]
    got = (outn, oo.astype(np.uint32), ol.cpu().numpy().astype(np.uint32), st.cpu().numpy())
    compare_batches(got, ref, f"masked tails, {kernel} kernel, {n} literals, base +{shift}")
    assert (g[: GUARD + shift] == SENT).all(), "bytes written before the output"
    assert (g[GUARD + shift + int(oo[-1]) :] == SENT).all(), "bytes written past the output"


@pytest.mark.parametrize("kernel", ["wave", "fill"])
@pytest.mark.parametrize("n", [4096, 300])
def test_masked_tails_compact_form(codec, n, kernel):
    """hpk_decode_batch_compact: every literal's bytes, length and status; nothing outside [0, out_off[n])."""
    from loona_amd.batch import compact_capacity

    blob, off, ref = _batch(n)
    codec.set_decode_kernel(kernel)
    need = compact_capacity(int(blob.size), n)
    big = torch.full((GUARD + need + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    out = big[GUARD : GUARD + need]
    out, oo, ol, st = codec.decode_compact(_dev(blob), _dev(off.astype(np.int32)), out_blob=out, sync=True)
    codec.set_decode_kernel("auto")
    g = big.cpu().numpy()
    o = oo.cpu().numpy().astype(np.uint32)
    end = int(o[n])
    assert end <= need
    got = (g[GUARD : GUARD + need], o, ol[:n].cpu().numpy().astype(np.uint32), st[:n].cpu().numpy())
    compare_batches(got, ref, f"masked tails, compacted form, {kernel} kernel, {n} literals")
    assert (g[:GUARD] == SENT).all(), "bytes written before the output"
    assert (g[GUARD + end :] == SENT).all(), "bytes written past the reported span"
    # the literals' byte ranges are disjoint
    ln = got[2].astype(np.int64)
    s = o[:n].astype(np.int64)[ln > 0]
    e = s + ln[ln > 0]
    order = np.argsort(s)
    assert (s[order][1:] >= e[order][:-1]).all(), "compacted literals overlap"
