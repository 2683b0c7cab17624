// hpk_walk.h — everything a single lane needs to decode a literal: the lane walk every decode kernel
// uses (hpk_wave.h, hpk_fill.h, hpk_long.h) and the code-by-code byte path. Plain per-lane code: the
// including file provides the HIP runtime, or tests/emu/shim.h (which stands in for the handful of
// builtins used here) when tests/emu replays these functions on the CPU against the oracle.
//   * Lane walk (v12): a lane holds its bit position as X = P + 31 and the dword pair (d0, d1) =
//     window dwords (X >> 5) - 1 and X >> 5, plus the next dword d2. The 32 bits at P are ONE
//     v_alignbit_b32(d0, d1, ~X). A step does two lookups in the two-symbol table (LUT2 / LUT3 layout,
//     hpk_code.h; 12 index bits, or 13 in the wave kernel: lut_bits), each decoding up to two codes of <= 12
//     (13) bits, and advances <= 24 (26) bits, so it crosses
//     at most one dword: the pair then slides by one (v_cndmask) and d2 takes d3, the dword read at the
//     top of the step. A code longer than 12 bits (EOS included) takes the rarely taken branch: one
//     leading-ones lookup. Bits past a literal's end are never masked: a code that runs past the end is,
//     by prefix-freeness, longer than what is left whatever follows, so the walk stops exactly where
//     huffman.rs's bit iterator stops matching (huffman.rs:100-123); the final padding check
//     (huffman.rs:128-160) looks at the residual bits only.
//   * Stores (v14): a checked step's (up to) four byte stores are unconditional, a byte that is not
//     output going to the lane's dummy slot (no exec-mask branch around each ds_write_b8).
//   * Masked tail (v38, the wave kernel): a literal's last <= 28 bits in four lookups on the bits with
//     ones past the literal's end, no fit test per code (lit12_tail, below); the checked step stays for
//     the lanes it leaves as slow and for the other kernels.
#pragma once
#include <stdint.h>

#include "../../include/hpk.h"
#include "hpk_code.h"

namespace hpkdec {

enum StoreMode { kDword = 0, kNoStore = 1, kChecked = 3, kPred = 4 };  // kPred: kDword, lane steps store
// unconditionally, a byte that is not output going to a per-lane dummy slot

// diagnostic mode 4 (kChecked): record the first out-of-region store instead of performing it
#ifdef __HIPCC__
__device__ unsigned long long g_chk[8];
__device__ __forceinline__ void chk_report(uint32_t code, uint32_t a0, uint32_t a1, uint32_t a2) {
    if (atomicCAS(&g_chk[0], 0ull, (unsigned long long)code) == 0ull) {
        g_chk[1] = a0;
        g_chk[2] = a1;
        g_chk[3] = a2;
        g_chk[4] = blockIdx.x;
        g_chk[5] = threadIdx.x;
    }
}
#else
inline void chk_report(uint32_t, uint32_t, uint32_t, uint32_t) {}
#endif

__device__ __forceinline__ void put8(uint8_t* __restrict__ out8, uint32_t pos, uint32_t v, uint32_t oend, int kStore) {
    if (kStore == kChecked) {
        if (pos < oend)
            out8[pos] = (uint8_t)v;
        else
            chk_report(1, pos, oend, 0);
    } else if (kStore == kDword || kStore == kPred) {
        out8[pos] = (uint8_t)v;
    } else {
        asm volatile("" ::"v"(v));
    }
}

// The 32 window bits at bit position p (big-endian dwords).
__device__ __forceinline__ uint32_t win_at(const uint32_t* __restrict__ win32, uint32_t p) {
    const uint32_t x = p + 31u;
    const uint32_t* q = win32 + (x >> 5);
    return __builtin_amdgcn_alignbit(q[-1], q[0], ~x);
}

// The two-symbol table a walk reads, kTab (hpk_code.h): 2 = LUT2 and 3 = LUT3, both of HPK_LUT_BITS = 12
// index bits; 4 = the LUT3 layout at HPK_LUT13_BITS = 13 index bits (decode v39, the wave kernel and its
// phases). Everything that depends on the index width takes it from here.
template <int kTab>
constexpr uint32_t lut_bits() {
    static_assert(kTab >= 2 && kTab <= 4, "table kind");
    return kTab == 4 ? (uint32_t)HPK_LUT13_BITS : (uint32_t)HPK_LUT_BITS;
}
template <int kTab>
constexpr bool lut_l3() {  // the entry layout is LUT3's
    return kTab >= 3;
}

// The codes one table entry decodes with rem bits left: ok1 / ok2 = its first / second code fits
// inside the literal; returns the bits they use.
template <int kTab = 2>
__device__ __forceinline__ uint32_t lut12(uint32_t e, uint32_t rem, bool& ok1, bool& ok2) {
    // a length field the entry does not hold is 15, past any clamped rem (and t1 >= l1: ok2 => ok1)
    static_assert(lut_bits<kTab>() < HPK_LUT2_CLAMP, "a held length is below the clamp");
    const uint32_t rc = min(rem, HPK_LUT2_CLAMP);
    if (lut_l3<kTab>()) {
        const uint32_t l1 = HPK_L3_LEN0(e), t1 = HPK_L3_HELD(e);
        ok1 = l1 <= rc;
        ok2 = (t1 <= rc) & (e < HPK_L3_NOTTWO);
        return ok2 ? t1 : (ok1 ? l1 : 0u);
    }
    const uint32_t l1 = HPK_L2_LEN0(e), t1 = HPK_L2_LEN01(e);
    ok1 = l1 <= rc;
    ok2 = t1 <= rc;
    return ok2 ? t1 : (ok1 ? l1 : 0u);
}
template <int kTab>
__device__ __forceinline__ bool lut_nottwo(uint32_t e) {
    return lut_l3<kTab>() ? e >= HPK_L3_NOTTWO : e >= HPK_LUT2_NOTTWO;
}
// An entry's second symbol byte, in place for a byte store (LUT2 / LUT3: [23:16])
template <int kTab>
__device__ __forceinline__ uint32_t lut_sym1(uint32_t e) {
    return e >> 16;
}

// Final status at a stop with rem residual bits and window w there (huffman.rs:128-160): at most
// 7 residual bits, all ones (the most significant bits of EOS).
__device__ __forceinline__ uint32_t residual_status(uint32_t rem, uint32_t w) {
    if (rem == 0) return HPK_OK;
    if (rem > 7) return HPK_PADDING_TOO_LARGE;
    return (w | (0xFFFFFFFFu >> rem)) != 0xFFFFFFFFu ? HPK_INVALID_PADDING : HPK_OK;
}

// Decode one code of any length from the window (>= 30 loaded bits): leading-ones table.
__device__ __forceinline__ void lo_decode(uint32_t w, const uint16_t* __restrict__ lo, uint32_t& sym,
                                          uint32_t& len, bool& eos) {
    const uint32_t kk = __clz(~w);
    const uint32_t e = lo[min(kk, (uint32_t)HPK_LO_RUNS - 1) * 32 + ((w << ((kk + 1) & 31)) >> 27)];
    eos = kk >= HPK_LO_RUNS || (e & 0x1FFu) == HPK_EOS;
    sym = e & 0xFFu;
    len = eos ? 30u : (e >> 9);
}

// ------------------------------------------------------------------------------------------
// Lane-per-literal walk.

struct Lit12 {
    uint32_t X;           // bit position in the window + 31
    uint32_t Eb;          // end bit position + 31: rem = Eb - X bits left
    uint32_t d0, d1, d2;  // window dwords (X >> 5) - 1, X >> 5, (X >> 5) + 1
    uint32_t o;           // next output byte in the LDS image
    uint32_t o0;          // first output byte of the literal
    uint32_t oend;        // checked mode: end of the literal's capacity
    uint32_t st;          // hpk_status set by the walk (EOS, or padding found by the long-code branch)
    uint32_t idx;         // literal index in the fill
    bool prog;            // the last step consumed a code or took the long-code branch
    bool more;            // (kMore steps) the walk may go on: the last step used both entries whole, or
                          // decoded a long code; false once a step has proved that no code fits
    bool act;             // holds a fast-path literal not yet finalised
};

// (Re)load the pair and the next dword at X.
// Contract: reads win32[(X >> 5) - 1], the dword BEFORE the one holding X, as well as that one and the next. With
// P = X - 31 the first bit wanted, that dword lies in front of the window exactly when P is the window's first bit
// (a literal at byte 0 of a dword-aligned window): then X % 32 == 31, every use of d0 is alignbit(d0, d1, ~X) with a
// shift of ~X & 31 == 0, which returns d1, and the first step that advances crosses a dword and replaces d0 by d1. So
// its value never reaches a result, but the callers keep it addressable (win_at reads the same dword):
//   hpk_wave.h          win32 is the LDS array's base and X carries the wave's offset (wbits): the dword is the last
//                       one of the dummy area (kWaveOff = kDummyOff + 256) for wave 0, else of the previous wave's image;
//   hpk_fill.h          win32 = smem + kInOff: the last dword of the two-symbol table (kInOff = kTabBytes + kLutBytes);
//   hpk_persist_lit.h   a lane's input slot starts with a pad dword for this read (sb >= 32; never written, never used);
//   hpk_long.h          its own copy of this load: ring[((j - 1) & (kRing - 1)) * kBlock] wraps inside the lane's ring;
//   hpk_huge_piece.h    does not load pairs: HugeWalk only reads forward, 16-byte chunks clamped to the batch's last one.
// The lane replays (tests/emu/emu.cpp, tail_emu.cpp, walk13_emu.cpp, tailword_emu.cpp) run every fill with that dword all
// zeros and all ones and require the same lengths, statuses and image; under a host sanitizer it is the first dword of
// the window's allocation.
__device__ __forceinline__ void lit12_load(Lit12& L, const uint32_t* __restrict__ win32) {
    const uint32_t* p = win32 + (L.X >> 5);
    L.d0 = p[-1];
    L.d1 = p[0];
    L.d2 = p[1];
}

// lit12_step's first part: the two lookups and their stores; returns whether a 13..30-bit code or EOS
// starts at the new position (lit12_park then does its leading-ones lookup).
template <int kStore, bool kP1, int kTab, bool kMore>
__device__ __forceinline__ bool lit12_step_main(Lit12& L, const uint32_t* __restrict__ win32,
                                                const uint32_t* __restrict__ lut, uint8_t* __restrict__ out8,
                                                uint32_t dmy) {
    const uint32_t d3 = win32[(L.X >> 5) + 2];  // the dword after d2, in case this step crosses one
    const uint32_t w = __builtin_amdgcn_alignbit(L.d0, L.d1, ~L.X);
    const uint32_t rem = L.Eb - L.X;
    const uint32_t e1 = lut[w >> (32 - lut_bits<kTab>())];
    bool a1, a2;
    const uint32_t u1 = lut12<kTab>(e1, rem, a1, a2);
    uint32_t use = u1;
    // a code longer than 12 bits (or EOS) starts here and may still fit (with more than 12 bits
    // left, any code the entry holds fits: no first code <=> the entry has none)
    bool park = !a1 & (rem > lut_bits<kTab>());
    bool more2 = false;
    if (kStore == kPred) {
        out8[a1 ? L.o : dmy] = (uint8_t)e1;
        if (kP1)
            (out8 + 1)[a2 ? L.o : dmy - 1u] = (uint8_t)lut_sym1<kTab>(e1);
        else
            out8[a2 ? L.o + 1 : dmy] = (uint8_t)lut_sym1<kTab>(e1);
    } else {
        if (a1) put8(out8, L.o, e1, L.oend, kStore);
        if (a2) put8(out8, L.o + 1, lut_sym1<kTab>(e1), L.oend, kStore);
    }
    L.o += (uint32_t)a1 + (uint32_t)a2;
    {
        // the first entry was consumed whole: look the next bits up too
        const bool cont = a1 & (a2 | lut_nottwo<kTab>(e1));
        const uint32_t w2 = w << u1;
        const uint32_t rem2 = rem - u1;
        const uint32_t e2 = lut[w2 >> (32 - lut_bits<kTab>())];
        bool b1, b2;
        const uint32_t u2 = lut12<kTab>(e2, rem2, b1, b2);
        park |= cont & !b1 & (rem2 > lut_bits<kTab>());
        b1 &= cont;
        b2 &= cont;
        // both entries used whole: more codes may follow (otherwise one of them held a code that does
        // not fit, or none with <= 12 bits left: the walk has ended here, huffman.rs:100-123)
        more2 = b1 & (b2 | lut_nottwo<kTab>(e2));
        if (kStore == kPred) {
            out8[b1 ? L.o : dmy] = (uint8_t)e2;
            if (kP1)
                (out8 + 1)[b2 ? L.o : dmy - 1u] = (uint8_t)lut_sym1<kTab>(e2);
            else
                out8[b2 ? L.o + 1 : dmy] = (uint8_t)lut_sym1<kTab>(e2);
        } else {
            if (b1) put8(out8, L.o, e2, L.oend, kStore);
            if (b2) put8(out8, L.o + 1, lut_sym1<kTab>(e2), L.oend, kStore);
        }
        L.o += (uint32_t)b1 + (uint32_t)b2;
        use += cont ? u2 : 0u;
    }
    const uint32_t xn = L.X + use;
    const bool cross = (xn ^ L.X) > 31u;
    L.d0 = cross ? L.d1 : L.d0;
    L.d1 = cross ? L.d2 : L.d1;
    L.d2 = cross ? d3 : L.d2;
    L.X = xn;
    L.prog = a1 | park;
    if (kMore) L.more = park | more2;
    return park;
}

template <int kStore, bool kMore>
__device__ __forceinline__ void lit12_park(Lit12& L, const uint32_t* __restrict__ win32, const uint16_t* __restrict__ lo,
                                           uint8_t* __restrict__ out8) {
    // a 13..30-bit code or EOS: one leading-ones lookup (any code in one read)
    const uint32_t wp = __builtin_amdgcn_alignbit(L.d0, L.d1, ~L.X);
    uint32_t s, len;
    bool eos;
    lo_decode(wp, lo, s, len, eos);
    const uint32_t r = L.Eb - L.X;
    if (len > r) {  // nothing fits in the > 12 bits left: huffman.rs:128-134
        L.st = HPK_PADDING_TOO_LARGE;
        L.Eb = L.X;
        if (kMore) L.more = false;
    } else if (eos) {  // huffman.rs:112-116
        L.st = HPK_EOS_IN_STRING;
        L.Eb = L.X;
        if (kMore) L.more = false;
    } else {
        put8(out8, L.o, s, L.oend, kStore);
        L.o += 1;
        L.X += len;
        lit12_load(L, win32);
    }
}

// One step: two lookups (up to four codes of <= 12 bits) and, for a longer code, one leading-ones
// lookup. kStore == kPred: the (up to) four byte stores are unconditional, a byte that is not output
// going to the lane's dummy slot out8[dmy] (no exec-mask branch around each store); kChecked
// (diagnostic mode 4) checks every store against the literal's capacity, kNoStore (mode 2) stores
// nothing.
template <int kStore, bool kP1 = false,   // kP1: a lookup's second byte stored at (address) + 1 by the
          int kTab = 2,                  // store's offset (the wave kernel; in the fill kernel's
          bool kMore = false>            // register budget the extra live dmy - 1 spills); kTab: lut12;
                                         // kMore: set L.more (the tails of decode v27)
__device__ __forceinline__ void lit12_step(Lit12& L, const uint32_t* __restrict__ win32, const uint32_t* __restrict__ lut,
                                           const uint16_t* __restrict__ lo, uint8_t* __restrict__ out8,
                                           uint32_t dmy = 0) {
    if (lit12_step_main<kStore, kP1, kTab, kMore>(L, win32, lut, out8, dmy)) lit12_park<kStore, kMore>(L, win32, lo, out8);
}

// Body step (decode v27): the same two lookups with NO fit tests, for a literal with at least
// kBodyMin bits left before the step. A step consumes <= 24 bits, so every code the two entries hold
// ends inside the literal, and >= 13 bits are left after it. The stores are unconditional at the
// lane's own output positions: an entry's second byte when it holds one code (or both bytes when it
// holds none) is garbage that the next store overwrites, or lies past the decoded bytes inside the
// literal's own region (see kBodyMin). Lengths come from the entries' "bits held" and "codes held" fields: ~25 VALU per
// step against lit12_step's ~48. A lookup that holds no code (a 13..30-bit code or EOS) takes the
// checked leading-ones branch of lit12_step; `body` says whether the next step may be a body step.
// kBodyMin is the 24 bits a step may consume + 5: after a body step >= 5 bits are left, so when the decoded bytes end
// there the decoded length is below the bound (a code is >= 5 bits) and a garbage byte at the next
// output position stays in the region; a lookup holding no code has >= 29 - 12 > 12 bits left, so it
// always takes the leading-ones branch (whose symbol overwrites the garbage)
constexpr uint32_t kBodyMin = 29;
// The same for a table of b index bits is 2 b + 5 (12 bits: the 29 above; 13 bits: 31). A step then consumes
// <= 2 b <= 26 bits, so it still crosses at most one dword and leaves >= 5 bits, and a lookup holding no code
// has >= b + 5 > b bits left (13 bits: >= 18 > 13).
template <int kTab>
constexpr uint32_t body_min() {
    return lut_bits<kTab>() == (uint32_t)HPK_LUT_BITS ? kBodyMin : 2u * lut_bits<kTab>() + 5u;
}

// kDup (diagnostic builds, LDS bank-conflict attribution): one access class of the step issued twice,
// the extra access a volatile one through an LDS-qualified pointer (a volatile access through a generic
// pointer became a flat access, and a later plain store to the same byte let the compiler drop the
// earlier one): 1 the two table reads, 2 the window read, 3 the four byte stores (the same bytes, the
// duplicate first). The conflict cycles a variant adds over the product are that class's.
#ifndef HPK_LDS_AS
#define HPK_LDS_AS __attribute__((address_space(3)))
#endif
// lit12_body's first part: the two lookups, their stores and the advance; returns u2, the bits the second
// entry holds (0: a code longer than the table's index, or EOS, starts at the new X; lit12_body_long)
template <int kStore, int kTab = 2, int kDup = 0>
__device__ __forceinline__ uint32_t lit12_body_main(Lit12& L, const uint32_t* __restrict__ win32,
                                                    const uint32_t* __restrict__ lut, uint8_t* __restrict__ out8) {
    const uint32_t d3 = win32[(L.X >> 5) + 2];
    if (kDup == 2) asm volatile("" ::"v"(((const volatile HPK_LDS_AS uint32_t*)win32)[(L.X >> 5) + 2]));
    const uint32_t w = __builtin_amdgcn_alignbit(L.d0, L.d1, ~L.X);
    const uint32_t e1 = lut[w >> (32 - lut_bits<kTab>())];
    const uint32_t u1 = lut_l3<kTab>() ? HPK_L3_HELD(e1) : HPK_L2_HELD(e1);
    const uint32_t e2 = lut[(w << u1) >> (32 - lut_bits<kTab>())];
    if (kDup == 1) {
        const volatile HPK_LDS_AS uint32_t* vl = (const volatile HPK_LDS_AS uint32_t*)lut;
        asm volatile("" ::"v"(vl[w >> (32 - lut_bits<kTab>())]));
        asm volatile("" ::"v"(vl[(w << u1) >> (32 - lut_bits<kTab>())]));
    }
    const uint32_t u2 = lut_l3<kTab>() ? HPK_L3_HELD(e2) : HPK_L2_HELD(e2);
    const uint32_t o1 = L.o + (lut_l3<kTab>() ? HPK_L3_CODES(e1) : HPK_L2_CODES(e1));
    if (kStore != kNoStore) {
        if (kDup == 3) {
            volatile HPK_LDS_AS uint8_t* v8 = (volatile HPK_LDS_AS uint8_t*)out8;
            v8[L.o] = (uint8_t)e1;
            (v8 + 1)[L.o] = (uint8_t)lut_sym1<kTab>(e1);
            v8[o1] = (uint8_t)e2;
            (v8 + 1)[o1] = (uint8_t)lut_sym1<kTab>(e2);
        }
        out8[L.o] = (uint8_t)e1;
        (out8 + 1)[L.o] = (uint8_t)lut_sym1<kTab>(e1);
        out8[o1] = (uint8_t)e2;
        (out8 + 1)[o1] = (uint8_t)lut_sym1<kTab>(e2);
    }
    L.o = o1 + (lut_l3<kTab>() ? HPK_L3_CODES(e2) : HPK_L2_CODES(e2));
    const uint32_t xn = L.X + u1 + u2;
    const bool cross = (xn ^ L.X) > 31u;
    L.d0 = cross ? L.d1 : L.d0;
    L.d1 = cross ? L.d2 : L.d1;
    L.d2 = cross ? d3 : L.d2;
    L.X = xn;
    return u2;
}

// lit12_body's second part, after a second lookup that held no code (nor the first, if u1 == 0): a code longer
// than the table's index or EOS at X; more bits than the index are left (>= body_min - index bits before that
// lookup), so the leading-ones branch of lit12_step applies
template <int kStore>
__device__ __forceinline__ void lit12_body_long(Lit12& L, const uint32_t* __restrict__ win32, const uint16_t* __restrict__ lo,
                                                uint8_t* __restrict__ out8) {
    const uint32_t wp = __builtin_amdgcn_alignbit(L.d0, L.d1, ~L.X);
    uint32_t sy, len;
    bool eos;
    lo_decode(wp, lo, sy, len, eos);
    const uint32_t r = L.Eb - L.X;
    if (len > r) {  // nothing fits in the > 12 (13) bits left: huffman.rs:128-134
        L.st = HPK_PADDING_TOO_LARGE;
        L.Eb = L.X;
    } else if (eos) {  // huffman.rs:112-116
        L.st = HPK_EOS_IN_STRING;
        L.Eb = L.X;
    } else {
        if (kStore != kNoStore) out8[L.o] = (uint8_t)sy;
        L.o += 1;
        L.X += len;
        lit12_load(L, win32);
    }
}

template <int kStore, int kTab = 2, int kDup = 0>
__device__ __forceinline__ void lit12_body(Lit12& L, const uint32_t* __restrict__ win32, const uint32_t* __restrict__ lut,
                                           const uint16_t* __restrict__ lo, uint8_t* __restrict__ out8, bool& body) {
    if (lit12_body_main<kStore, kTab, kDup>(L, win32, lut, out8) == 0u) lit12_body_long<kStore>(L, win32, lo, out8);
    body = L.Eb - L.X >= body_min<kTab>();
}

// A round of kSteps body steps (decode v41, the wave kernel's lane loop). The steps are NESTED: step s + 1 lives
// inside step s's `if (body)`. Within a round `body` only goes from true to false, so the active lanes only
// narrow and every step's region ends at the one join behind the round: a step costs one compare and one
// narrowing of exec, and no value of the walk is live out of a step in a second register. kDefer says what a
// step does with a second lookup that holds no code (a 13..30-bit code or EOS at the new X):
//   0  the leading-ones block inline, as lit12_body does;
//   1  the lane is parked: it has advanced by u1 + u2 and stored its (harmless) bytes, and drops out of the rest
//      of the round like a lane whose body ended;
//   2  the lane is parked and stays in the round while >= body_min bits are left: a body step at a position
//      where no code of <= index bits starts holds u1 = u2 = 0, so it moves nothing and stores the two garbage
//      bytes at o and o + 1 that the step before it (or lit12_body's u1 == 0 case) stores there anyway; the
//      lane is parked exactly when its last executed step's second lookup held no code.
// Behind a deferred round ONE test, wave-wide by the caller's `any` (the CPU replay: the lane's own flag), runs
// the leading-ones block for the parked lanes and recomputes their `body`: a parked lane's next action is the
// lookup lit12_body would have done, from the same state, so the results are the same byte for byte and only the
// slot in which it happens moves (a parked lane loses at most kSteps - 1 step slots).
template <int kStore, int kTab, int kDefer, int kDup, int kLeft>
__device__ __forceinline__ void lit12_round_steps(Lit12& L, const uint32_t* __restrict__ win32,
                                                  const uint32_t* __restrict__ lut, const uint16_t* __restrict__ lo,
                                                  uint8_t* __restrict__ out8, bool go, uint32_t& u2) {
    if (go) {
        u2 = lit12_body_main<kStore, kTab, kDup>(L, win32, lut, out8);
        if (kDefer == 0 && u2 == 0u) lit12_body_long<kStore>(L, win32, lo, out8);
        if constexpr (kLeft > 1) {
            go = L.Eb - L.X >= body_min<kTab>();
            if (kDefer == 1) go &= u2 != 0u;
            lit12_round_steps<kStore, kTab, kDefer, kDup, kLeft - 1>(L, win32, lut, lo, out8, go, u2);
        }
    }
}

// `body` is, before and after the round, whether the lane's next step may be a body step: L.Eb - L.X >= body_min
// (made from the state behind the round, so that no flag is carried through the steps)
template <int kStore, int kTab, int kSteps, int kDefer, int kDup = 0, class Any>
__device__ __forceinline__ void lit12_round(Lit12& L, const uint32_t* __restrict__ win32, const uint32_t* __restrict__ lut,
                                            const uint16_t* __restrict__ lo, uint8_t* __restrict__ out8, bool& body,
                                            Any any) {
    uint32_t u2 = 1u;  // the second lookup's bits held, of the lane's last executed step (no step: not parked)
    lit12_round_steps<kStore, kTab, kDefer, kDup, kSteps>(L, win32, lut, lo, out8, body, u2);
    if (kDefer != 0) {
        const bool parked = u2 == 0u;
        if (any(parked)) {
            if (parked) lit12_body_long<kStore>(L, win32, lo, out8);
        }
    }
    body = L.Eb - L.X >= body_min<kTab>();
}

// Masked tail (decode v38): the last bits of a literal, rem = Eb - X <= 28 of them (0: an empty slot, or
// a walk that ended in its body with a status), in straight-line code with no fit test per code and no
// window read after lit12_load. The bits past the literal's end are set to ones: the stream then ends in
// an all-ones run, which prefixes only EOS (30 bits), so for a valid literal plain lookups find exactly
// the real codes and then "no code". Four lookups are enough: an entry holds a single code only when that
// code and the next one take >= 13 bits together (an entry with two codes holds >= 10), so two lookups
// that both hold a code consume >= 13 bits, four >= 26, and no code fits in the <= 2 bits then left; a
// lookup that holds no code leaves the position where it is, and so do the lookups after it.
//   * An entry is accepted while consumed + held <= rem: its codes then lie inside the literal, they are
//     the codes the checked walk decodes, and their bytes go to o and o + 1. Every other byte (one the
//     entry does not hold, or any byte of a rejected entry: a code completed by the ones past the end)
//     goes to the lane's dummy slot, so a tail never stores outside the literal's region, whatever the
//     input.
//   * r = rem - consumed bits are left. A rejected entry (r wraps) or r >= 13 (a 13..28-bit code may
//     start there and fit) makes the lane `slow`: its state is left as it was, and the caller runs the
//     checked steps (lit12_step<.., kMore>) from it; the bytes already stored are the ones those steps
//     store again. Otherwise no code fits in the r <= 12 bits left (a <= 12-bit code inside them would
//     have been found), and the walk has ended: X moves there, st is the residual bits' status unless
//     the body set one, and Eb = X (as after a status in the body: lit12_status then returns st).
// With the 13-bit table (kTab 4, decode v39) a tail holds <= 30 bits (body_min is 31), still one register. An
// entry then holds a single code only when that code and the next one take >= 14 bits together (an entry with
// two codes holds >= 10), so two lookups that both hold a code consume >= 14 bits, four >= 28, and no code fits
// in the <= 2 bits then left: four lookups still suffice. A lane is slow at r >= 14 (a 14..30-bit code may start
// there and fit); in r <= 13 bits a code would have been found.
// The state lives inverted (n = ~bits: zeros past the end), so a shift by `held` fills with ones also
// when held is 0 (v_alignbit_b32 by 32 - held would return the fill word). ~14 VALU, one table read and
// two byte stores per lookup, against the ~48 / 2 / 4 of a checked step, of which a tail took two.
struct Tail12 {
    uint32_t n;     // ~(the 32 bits at X + used), zeros past the literal's end
    uint32_t used;  // bits the lookups hold so far
    uint32_t o;     // next output byte
    uint32_t rem;   // bits left at the tail's start
};

__device__ __forceinline__ void tail12_begin(Tail12& T, const Lit12& L) {
    T.rem = L.Eb - L.X;
    T.n = ~__builtin_amdgcn_alignbit(L.d0, L.d1, ~L.X) & ~(0xFFFFFFFFu >> T.rem);
    T.used = 0;
    T.o = L.o;
}

// The tail's state word alone, made where the lane still holds its dword pair (the wave kernel saves it when a
// lane's first literal leaves its body, fill trim A): Tail12::n as tail12_begin makes it from the same state.
// rem = Eb - X <= 30 there (0 after a status in the body, or in an empty slot: the word is then 0).
__device__ __forceinline__ uint32_t tail12_word(const Lit12& L) {
    return ~__builtin_amdgcn_alignbit(L.d0, L.d1, ~L.X) & ~(0xFFFFFFFFu >> (L.Eb - L.X));
}
// tail12_begin from a saved word: no dword of the window is needed (nor loaded) for the masked tail
__device__ __forceinline__ void tail12_begin_saved(Tail12& T, uint32_t n, uint32_t rem, uint32_t o) {
    T.rem = rem;
    T.n = n;
    T.used = 0;
    T.o = o;
}

template <int kStore, int kTab>
__device__ __forceinline__ void tail12_look(Tail12& T, const uint32_t* __restrict__ lut, uint8_t* __restrict__ out8,
                                            uint32_t dmy) {
    const uint32_t e = lut[(T.n >> (32 - lut_bits<kTab>())) ^ ((1u << lut_bits<kTab>()) - 1u)];
    const uint32_t held = lut_l3<kTab>() ? HPK_L3_HELD(e) : HPK_L2_HELD(e);
    T.used += held;
    const uint32_t codes = T.used <= T.rem ? (lut_l3<kTab>() ? HPK_L3_CODES(e) : HPK_L2_CODES(e)) : 0u;
    if (kStore != kNoStore) {
        out8[codes >= 1u ? T.o : dmy] = (uint8_t)e;
        (out8 + 1)[codes >= 2u ? T.o : dmy - 1u] = (uint8_t)lut_sym1<kTab>(e);
    }
    T.o += codes;
    T.n <<= held;
}

// returns whether the lane is slow (L is then unchanged)
template <int kTab = 2>
__device__ __forceinline__ bool tail12_end(const Tail12& T, Lit12& L) {
    const uint32_t r = T.rem - T.used;
    const bool slow = r > lut_bits<kTab>();
    const uint32_t st = r == 0u ? HPK_OK : (r > 7u ? HPK_PADDING_TOO_LARGE : (T.n != 0u ? HPK_INVALID_PADDING : HPK_OK));
    L.X = slow ? L.X : L.X + T.used;
    L.o = slow ? L.o : T.o;
    L.st = slow || L.st != HPK_OK ? L.st : st;
    L.Eb = slow ? L.Eb : L.X;
    return slow;
}

template <int kStore, int kTab>
__device__ __forceinline__ bool lit12_tail(Lit12& L, const uint32_t* __restrict__ lut, uint8_t* __restrict__ out8,
                                           uint32_t dmy) {
    Tail12 T;
    tail12_begin(T, L);
#pragma unroll
    for (int i = 0; i < 4; ++i) tail12_look<kStore, kTab>(T, lut, out8, dmy);
    return tail12_end<kTab>(T, L);
}

// Final status of a literal whose walk has stopped; a status set by the walk wins.
__device__ __forceinline__ uint32_t lit12_status(const Lit12& L) {
    if (L.st != HPK_OK) return L.st;
    return residual_status(L.Eb - L.X, __builtin_amdgcn_alignbit(L.d0, L.d1, ~L.X));
}

// ------------------------------------------------------------------------------------------
// The code-by-code byte path: one literal decoded a code at a time into a byte destination with a
// capacity check per byte (a literal whose output region is below the decoded bound).

struct Lit {
    uint64_t win;   // next bits, MSB-aligned (bits past the literal: whatever follows)
    uint32_t nb;    // loaded bits in win
    uint32_t nxt;   // next source dword (raw), merged at the next refill
    uint32_t pf;    // the dword after it (raw, read one refill ahead)
    uint32_t q;     // source dword index of pf
    uint32_t rem;   // literal bits not yet consumed
    uint32_t cnt;   // bytes decoded
    uint32_t st;    // hpk_status
    uint64_t acc;   // (unread since the dword stores went; with accn kept, zeroed in lit_begin, because the fill
    uint32_t accn;  // kernel's diagnostic modes 2-4 allocate their registers differently without them)
    bool live;      // still decoding
};

// Bitstream sources: a staged LDS window (big-endian dwords), or global memory (clamped to the batch).
struct LdsSwapSrc {
    const uint32_t* p;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return __builtin_bswap32(p[i]); }
};
struct GlobalSrc {
    const uint32_t* p;
    uint32_t last;  // last dword index holding a byte of the batch: never read past it
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return p[min(i, last)]; }
};

template <class Src>
__device__ __forceinline__ void lit_begin(Lit& L, const Src& src, uint32_t sb, uint32_t nbytes) {
    L.rem = nbytes * 8u;
    L.cnt = 0;
    L.st = HPK_OK;
    L.live = nbytes != 0;
    L.acc = 0;
    L.accn = 0;
    const uint32_t q0 = sb >> 2;
    const uint32_t sk = (sb & 3u) * 8u;
    const uint32_t d0 = src(q0);
    L.nxt = src(q0 + 1);
    L.pf = src(q0 + 2);
    L.q = q0 + 2;
    L.win = ((uint64_t)__builtin_bswap32(d0) << 32) << sk;
    L.nb = 32u - sk;
}

// Top the window up to >= 32 bits from the prefetched dword; read the next one.
template <class Src>
__device__ __forceinline__ void lit_refill(Lit& L, const Src& src) {
    const bool need = L.nb <= 32u;
    const uint64_t add = (uint64_t)__builtin_bswap32(L.nxt) << ((32u - L.nb) & 63u);
    L.win |= need ? add : 0ull;
    L.nb += need ? 32u : 0u;
    L.nxt = need ? L.pf : L.nxt;
    L.q += need ? 1u : 0u;
    L.pf = src(L.q);
}

template <class Src, class Dst>
__device__ __forceinline__ void lit_bytes_to(Lit& L, const Src& src, const uint16_t* lo, Dst dst, uint32_t ocap,
                                             uint32_t sb, uint32_t nbytes) {
    lit_begin(L, src, sb, nbytes);
    while (L.live) {
        lit_refill(L, src);
        uint32_t sym, len;
        bool eos;
        lo_decode((uint32_t)(L.win >> 32), lo, sym, len, eos);
        if (len > L.rem) break;
        if (eos) {
            L.st = HPK_EOS_IN_STRING;
            break;
        }
        if (L.cnt >= ocap) {
            L.st = HPK_OUTPUT_OVERFLOW;
            break;
        }
        dst(L.cnt, (uint8_t)sym);
        L.cnt += 1;
        L.win <<= len;
        L.nb -= len;
        L.rem -= len;
        L.live = L.rem != 0u;
    }
}

__device__ __forceinline__ uint32_t lit_status(const Lit& L) {
    uint32_t st = L.st;
    if (st == HPK_OK && L.rem > 0) {
        if (L.rem > 7) {
            st = HPK_PADDING_TOO_LARGE;
        } else {
            const uint32_t w = (uint32_t)(L.win >> 32) | (0xFFFFFFFFu >> L.rem);
            if (w != 0xFFFFFFFFu) st = HPK_INVALID_PADDING;
        }
    }
    return st;
}

}  // namespace hpkdec
