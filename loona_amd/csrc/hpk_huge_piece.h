// hpk_huge_piece.h — the per-piece half of the huge-literal phase (hpk_huge.h has the algorithm and
// the workgroup's protocol): the walker over a literal in global memory and what one lane does for one
// piece. Plain per-lane code on hpk_walk.h alone (hpk_persist.h walks with it too; tests/emu replays it
// on the CPU).
#pragma once
#include "hpk_walk.h"

namespace hpkdec {

#ifndef HPK_HUGE_MIN
#define HPK_HUGE_MIN 8192u  // encoded bytes from which a literal is a huge one (config 3's longest: 3.4 KiB)
#endif
constexpr uint32_t kHugePieceMin = 64;  // bytes per piece at least
constexpr uint32_t kHugeTerm = 0x100u;  // piece flag: the walk ended in this piece (status in the low byte)
constexpr uint32_t kHugeNone = 0xFFFFFFFFu;
constexpr uint32_t kHugeLimit = 1u << 28;  // literal bit positions fit in 32 bits below this many bytes

// Walker over a literal in global memory: a 64-bit window (MSB first), the chunk holding the next
// dword to merge (c0) and the one after it (c1, loaded when c0 becomes current).
struct HugeWalk {
    uint64_t win;
    uint32_t nb;   // bits in win
    uint32_t qi;   // absolute dword index of the next dword to merge
    uint32_t pos;  // literal-relative bit position of win's first bit
    uint4 c0, c1;
};

// Dword j (0..3) of a chunk, by shifts: written as selects of its elements, the compiler made it a
// dynamically indexed vector access, kept the chunks in scratch memory and read them back from there.
__device__ __forceinline__ uint32_t huge_sel(const uint4& c, uint32_t j) {
    const uint32_t sh = (j & 1u) * 32u;
    const uint32_t lo = (uint32_t)((((uint64_t)c.y << 32) | c.x) >> sh);
    const uint32_t hi = (uint32_t)((((uint64_t)c.w << 32) | c.z) >> sh);
    return (j & 2u) ? hi : lo;
}

// ld16(ci): 16-byte chunk ci of the input (clamped to the batch's last chunk).
template <class Ld>
__device__ __forceinline__ void huge_begin(HugeWalk& W, const Ld& ld16, uint32_t lbyte, uint32_t pos) {
    const uint32_t b = lbyte + (pos >> 3);
    const uint32_t qd = b >> 2;
    const uint32_t sk = (b & 3u) * 8u + (pos & 7u);
    W.c0 = ld16(qd >> 2);
    W.c1 = ld16((qd >> 2) + 1u);
    W.win = ((uint64_t)__builtin_bswap32(huge_sel(W.c0, qd & 3u)) << 32) << sk;
    W.nb = 32u - sk;
    W.qi = qd + 1u;
    W.pos = pos;
    if ((W.qi & 3u) == 0u) {
        W.c0 = W.c1;
        W.c1 = ld16((W.qi >> 2) + 1u);
    }
}

// The next code at W.pos (>= 33 bits in the window after the refill): symbol, length, EOS; and when
// the table entry holds a second code too, its symbol and the two codes' length (held; else 0).
template <int kTab, class Ld>
__device__ __forceinline__ void huge_peek(HugeWalk& W, const Ld& ld16, const uint32_t* __restrict__ lut,
                                          const uint16_t* __restrict__ lo, uint32_t& sym, uint32_t& len, bool& eos,
                                          uint32_t& sym1, uint32_t& held) {
    if (W.nb <= 32u) {
        W.win |= (uint64_t)__builtin_bswap32(huge_sel(W.c0, W.qi & 3u)) << (32u - W.nb);
        W.nb += 32u;
        W.qi += 1u;
        if ((W.qi & 3u) == 0u) {
            W.c0 = W.c1;
            W.c1 = ld16((W.qi >> 2) + 1u);
        }
    }
    const uint32_t w = (uint32_t)(W.win >> 32);
    const uint32_t e = lut[w >> (32 - lut_bits<kTab>())];
    const uint32_t l0 = lut_l3<kTab>() ? HPK_L3_LEN0(e) : HPK_L2_LEN0(e);  // 15: no code within the index bits
    if (l0 <= lut_bits<kTab>()) {
        sym = e & 0xFFu;
        len = l0;
        eos = false;
        const uint32_t codes = lut_l3<kTab>() ? HPK_L3_CODES(e) : HPK_L2_CODES(e);
        held = codes == 2u ? (lut_l3<kTab>() ? HPK_L3_HELD(e) : HPK_L2_HELD(e)) : 0u;
        sym1 = (e >> 16) & 0xFFu;
    } else {
        lo_decode(w, lo, sym, len, eos);
        held = 0;
        sym1 = 0;
    }
}

__device__ __forceinline__ void huge_adv(HugeWalk& W, uint32_t len) {
    W.win <<= len;
    W.nb -= len;
    W.pos += len;
}

// Count the codes from W.pos up to the first code that starts at or after nx (last: to the walk's
// end). c: codes counted; returns the flag (kHugeTerm | status if the walk ended here, else 0).
template <int kTab, class Ld>
__device__ __forceinline__ uint32_t huge_count(HugeWalk& W, const Ld& ld16, const uint32_t* __restrict__ lut,
                                               const uint16_t* __restrict__ lo, uint32_t nbits, uint32_t nx, bool last,
                                               uint32_t& c) {
    c = 0;
    for (;;) {
        if (!last && W.pos >= nx) return 0u;
        uint32_t sym, len, sym1, held;
        bool eos;
        huge_peek<kTab>(W, ld16, lut, lo, sym, len, eos, sym1, held);
        const uint32_t rem = nbits - W.pos;
        if (held != 0u && held <= rem && (last || W.pos + len < nx)) {  // two codes, both counted here
            huge_adv(W, held);
            c += 2u;
            continue;
        }
        if (len > rem) return kHugeTerm | residual_status(rem, (uint32_t)(W.win >> 32));  // huffman.rs:128-160
        if (eos) return kHugeTerm | HPK_EOS_IN_STRING;                                  // huffman.rs:112-116
        huge_adv(W, len);
        c += 1u;
    }
}

// Piece geometry of a literal of nbytes: P pieces of PB bytes (the last one shorter, never empty),
// OV bits of lead before a piece's start.
__device__ __forceinline__ void huge_geometry(uint32_t nbytes, uint32_t lanes, uint32_t& P, uint32_t& PB, uint32_t& OV) {
    P = min(lanes, (nbytes + kHugePieceMin - 1u) / kHugePieceMin);
    PB = (nbytes + P - 1u) / P;
    P = (nbytes + PB - 1u) / PB;
    OV = PB >= 512u ? 512u : 256u;
}

// Pass 1 of piece k: S (first code start >= the piece's start; kHugeNone if the lead walk ended
// before it), E, c, flag.
template <int kTab, class Ld>
__device__ __forceinline__ void huge_pass1(const Ld& ld16, const uint32_t* __restrict__ lut, const uint16_t* __restrict__ lo,
                                           uint32_t lbyte, uint32_t nbytes, uint32_t k, uint32_t P, uint32_t PB,
                                           uint32_t OV, uint32_t& S, uint32_t& E, uint32_t& c, uint32_t& fl) {
    const uint32_t nbits = nbytes * 8u, st = k * PB * 8u;
    const bool last = k + 1u == P;
    const uint32_t nx = last ? nbits : (k + 1u) * PB * 8u;
    HugeWalk W;
    huge_begin(W, ld16, lbyte, k == 0u ? 0u : (st > OV ? st - OV : 0u));
    c = 0;
    fl = 0;
    while (W.pos < st) {  // the lead: codes before the piece's start, not counted
        uint32_t sym, len, sym1, held;
        bool eos;
        huge_peek<kTab>(W, ld16, lut, lo, sym, len, eos, sym1, held);
        if (held != 0u && held <= nbits - W.pos && W.pos + len < st) {  // two codes, both before the start
            huge_adv(W, held);
            continue;
        }
        if (len > nbits - W.pos || eos) {  // (a speculative walk that ends: the fix walks this piece again)
            S = E = kHugeNone;
            return;
        }
        huge_adv(W, len);
    }
    S = W.pos;
    fl = huge_count<kTab>(W, ld16, lut, lo, nbits, nx, last, c);
    E = W.pos;
}

// The fix: piece k walked again from `from` (its predecessor's E).
template <int kTab, class Ld>
__device__ __forceinline__ void huge_refix(const Ld& ld16, const uint32_t* __restrict__ lut, const uint16_t* __restrict__ lo,
                                           uint32_t lbyte, uint32_t nbytes, uint32_t k, uint32_t P, uint32_t PB,
                                           uint32_t from, uint32_t& S, uint32_t& E, uint32_t& c, uint32_t& fl) {
    const uint32_t nbits = nbytes * 8u;
    const bool last = k + 1u == P;
    const uint32_t nx = last ? nbits : (k + 1u) * PB * 8u;
    HugeWalk W;
    huge_begin(W, ld16, lbyte, from);
    S = from;
    fl = huge_count<kTab>(W, ld16, lut, lo, nbits, nx, last, c);
    E = W.pos;
}

// Pass 2 of a piece: its c codes from S, stored at output byte ob (absolute, out_base-relative):
// 8-byte stores of the whole 8-byte groups, the partial groups at the two ends bytewise.
template <int kTab, class Ld, class St8, class St1>
__device__ __forceinline__ void huge_pass2(const Ld& ld16, const uint32_t* __restrict__ lut, const uint16_t* __restrict__ lo,
                                           uint32_t lbyte, uint32_t S, uint32_t c, uint32_t ob, const St8& st8,
                                           const St1& st1) {
    HugeWalk W;
    huge_begin(W, ld16, lbyte, S);
    uint64_t acc = 0;
    uint32_t p = ob;
    auto emit = [&](uint32_t sym) {
        acc |= (uint64_t)sym << (8u * (p & 7u));
        if ((p & 7u) == 7u) {
            const uint32_t g = p - 7u;
            if (g >= ob) {
                st8(g, acc);
            } else {
                for (uint32_t x = ob; x <= p; ++x) st1(x, (uint8_t)(acc >> (8u * (x & 7u))));
            }
            acc = 0;
        }
        p += 1u;
    };
    for (uint32_t j = 0; j < c;) {
        uint32_t sym, len, sym1, held;
        bool eos;
        huge_peek<kTab>(W, ld16, lut, lo, sym, len, eos, sym1, held);
        emit(sym);
        if (held != 0u && j + 2u <= c) {  // (the codes pass 1 counted: both exist)
            emit(sym1);
            huge_adv(W, held);
            j += 2u;
        } else {
            huge_adv(W, len);
            j += 1u;
        }
    }
    for (uint32_t x = max(ob, p & ~7u); x < p; ++x) st1(x, (uint8_t)(acc >> (8u * (x & 7u))));
}

}  // namespace hpkdec
