"""Cases for the packed string-literal encode (hpk_encode_strings_packed, hpk_string_len_batch), shared by
test_encode_strings_plan.py (CPU: expected() agrees with hpack_ref, a placed case reaches the cut or edge it
claims) and test_gpu_encode_strings.py (the device result, byte for byte).

A case is (strs, policy, in_shift, out_shift): the plaintext literals, one policy per literal (or None = all
AUTO), and the misalignment of the input / output blob's first byte from a 16-byte boundary. The expected bytes
never come from the code under test: payloads are the C oracle's (oracle_encode_batch), prefixes are
hpack_ref.encode_integer's, put together by the rule of hpack_ref.Encoder._string (expected()).

The emit kernel cuts its tiles by hpk_encode2's rule (encode_cases.tile_plan) on the representations' offsets,
with its own geometry (hpk_test_strings_geometry): geometry() gives it as an encode_cases.Geo so that the
builders of encode_cases and encode_packed_cases place their literals against it."""

import collections
import ctypes
import functools

import numpy as np

import encode_cases as ec
import encode_packed_cases as pc
from hpk_util import hpack_ref, oracle_encode_batch, pack

AUTO, RAW, HUFFMAN, VERBATIM = 0, 1, 2, 3

Expected = collections.namedtuple("Expected", "blob in_off policy out_off out_len flat huff plen")


@functools.lru_cache(maxsize=None)
def geometry():
    """the emit kernel's geometry as an encode_cases.Geo (B, the input bytes per thread, is the encode kernel's:
    only thread_edges uses it)"""
    from loona_amd import _lib

    v = [ctypes.c_uint32(0) for _ in range(4)]
    assert _lib.lib().hpk_test_strings_geometry(*[ctypes.byref(x) for x in v]) == _lib.HPK_E_OK
    t, i, q, p = [x.value for x in v]
    return ec.Geo(t, i, q, ec.geometry().B, p)


def expected(strs, policy=None):
    """The answer to (strs, policy): per literal the 7-bit-prefix integer of the payload length
    (hpack_ref.encode_integer, leading 0x80 for the Huffman form) followed by the payload, the oracle's Huffman
    bytes or the literal itself; under VERBATIM the literal alone. AUTO takes the Huffman form iff the literal is
    non-empty and the oracle's encoding is strictly shorter (hpack_ref.Encoder._string). One oracle call."""
    n = len(strs)
    pol = np.zeros(n, np.uint8) if policy is None else np.asarray(policy, np.uint8)
    assert pol.shape == (n,) and (pol <= VERBATIM).all()
    blob, off = pack(strs)
    off = off.astype(np.int64)
    ob, oo, hl, st = oracle_encode_batch(blob, off.astype(np.uint32))
    assert not st.any()
    hl, oo = hl.astype(np.int64), oo.astype(np.int64)
    lens = np.diff(off)
    huff = (pol == HUFFMAN) | ((pol == AUTO) & (lens > 0) & (hl < lens))
    p = np.where(huff, hl, lens)
    # the prefixes: one encode_integer per distinct (payload length, form)
    keys, inv = np.unique(p * 2 + huff, return_inverse=True)
    tab = np.zeros((len(keys), 6), np.uint8)
    tlen = np.zeros(len(keys), np.int64)
    for j, key in enumerate(keys.tolist()):
        octets = hpack_ref.encode_integer(key >> 1, 7, 0x80 if key & 1 else 0)
        tab[j, : len(octets)] = list(octets)
        tlen[j] = len(octets)
    plen = np.where(pol == VERBATIM, 0, tlen[inv]) if n else np.zeros(0, np.int64)
    pre = tab[inv] if n else np.zeros((0, 6), np.uint8)
    out_len = plen + p
    out_off = np.zeros(n + 1, np.int64)
    np.cumsum(out_len, out=out_off[1:])
    flat = np.zeros(int(out_off[-1]), np.uint8)
    for j in range(6):
        m = plen > j
        flat[out_off[:-1][m] + j] = pre[m, j]
    tot = int(p.sum())
    if tot:
        cat = np.concatenate([blob, ob])
        payload = ec.gather(cat, np.where(huff, blob.size + oo[:n], off[:-1]), p)
        ends = np.cumsum(p)
        flat[np.repeat(out_off[:-1] + plen - (ends - p), p) + np.arange(tot)] = payload
    return Expected(blob, off, pol, out_off, out_len, flat, huff, plen)


def policies(n, pol):
    return np.full(n, pol, np.uint8)


# ---- the decision edge ------------------------------------------------------------------------------

# code lengths (RFC 7541 App. B): '0' 5, 'A' 6, 'B' 7, '&' 8, '*' 8, 'X' 8, 'Z' 8, '!' 10, '#' 12, '<' 15
_SYM = {5: b"0", 6: b"A", 7: b"B", 8: b"&"}


def with_bits(n, bits):
    """a literal of n bytes whose code bits sum to `bits`: 5- to 8-bit codes for 5 n <= bits <= 8 n (from n = 4
    on, 8 n - 8 is '&' x (n - 4) + 'A' x 4 and 8 n - 7 is 'B' + '&' x (n - 4) + 'A' x 3); 8 n + 1 is n - 2
    eight-bit codes, a 7-bit and a 10-bit one"""
    if bits == 8 * n + 1:
        assert n >= 2
        return b"&" * (n - 2) + b"B" + b"!"
    if n >= 4 and bits == 8 * n - 8:
        return b"&" * (n - 4) + b"A" * 4
    if n >= 4 and bits == 8 * n - 7:
        return b"B" + b"&" * (n - 4) + b"A" * 3
    assert 5 * n <= bits <= 8 * n
    out, left = [], bits
    for k in range(n):
        rest = n - k - 1
        ln = min(8, left - 5 * rest)
        out.append(_SYM[ln])
        left -= ln
    assert left == 0
    return b"".join(out)


def decision_edge():
    """for n in 3, 10, 127, 128: literals of n bytes with 8n-8 code bits (the H-bit form, n-1 bytes), 8n-7, 8n and
    8n+1 (raw: the Huffman form is not strictly shorter) -> (strs, the literals AUTO Huffman-codes)"""
    strs, huff = [], []
    for n in (3, 10, 127, 128):
        for bits in (8 * n - 8, 8 * n - 7, 8 * n, 8 * n + 1):
            strs.append(with_bits(n, bits))
            huff.append(bits == 8 * n - 8)
    return strs, np.array(huff)


# ---- prefix-length edges ----------------------------------------------------------------------------

def five_bit(nbytes, seed=0):
    rng = np.random.default_rng(21000 + seed)
    return bytes(rng.choice(np.frombuffer(ec.FIVE_BIT, np.uint8), nbytes).astype(np.uint8))


def huff_input_len(payload):
    """the bytes of 5-bit symbols whose Huffman coding is `payload` bytes: the largest such count"""
    return 8 * payload // 5


PREFIX_EDGES = (126, 127, 128, 254, 255, 16510, 16511)
PREFIX_EDGES_RAW_ONLY = (2097278, 2097279)


def prefix_edges_small():
    """raw payloads (under RAW, uniform bytes) and Huffman payloads (under AUTO, 5-bit symbols) of every prefix
    edge below 3 octets' end -> (strs, policy, payload lengths, forms)"""
    rng = np.random.default_rng(22000)
    strs, pol, pay, huff = [], [], [], []
    for p in PREFIX_EDGES:
        strs.append(ec._rand(rng, p))
        pol.append(RAW)
        pay.append(p)
        huff.append(False)
        strs.append(five_bit(huff_input_len(p), p))
        pol.append(AUTO)
        pay.append(p)
        huff.append(True)
    return strs, np.array(pol, np.uint8), np.array(pay), np.array(huff)


# ---- batches ------------------------------------------------------------------------------------------

def mixed_batch(n, hi, seed):
    """n literals of 0..hi bytes, text or uniform bytes, a random policy each"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, hi + 1, n)
    text = rng.random(n) < 0.5
    strs = [ec._text(rng, k) if t else ec._rand(rng, k) for k, t in zip(lens, text)]
    return strs, rng.integers(0, 4, n).astype(np.uint8)


def prefix_straddle():
    """40 literals with 2- and 3-octet prefixes (payloads of 127..400 bytes under RAW)"""
    rng = np.random.default_rng(23000)
    lens = [127, 128, 254, 255, 256, 300] * 6 + [400, 381, 382, 383]
    return [ec._rand(rng, k) for k in lens], policies(len(lens), RAW)


HEADER_CHARS = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789-./=; ", np.uint8)  # codes of 5 to 8 bits


def lone(nbytes, shift):
    """one literal of header-like text (its Huffman form is shorter: AUTO codes it)"""
    rng = np.random.default_rng(29000 + nbytes % 1000 + shift)
    return [bytes(rng.choice(HEADER_CHARS, nbytes).astype(np.uint8))]


def uniform_batch(n, hi, seed):
    rng = np.random.default_rng(seed)
    return [ec._rand(rng, k) for k in rng.integers(0, hi + 1, n)]


@functools.lru_cache(maxsize=None)
def multi_wg_expected():
    return expected(pc.multi_wg()[0])


def plan_of(strs, policy, in_shift, out_shift, geo):
    x = expected(strs, policy)
    assert len(strs) <= geo.P  # one workgroup: the model holds
    return ec.tile_plan(x.in_off, x.out_off, in_shift & 15, out_shift & 15, geo), x
