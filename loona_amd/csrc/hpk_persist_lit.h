// hpk_persist_lit.h — what one lane of the small-call mode's persistent kernel (hpk_persist.h) does for one
// literal: the staged walk (persist_literal_lds: the literal's chunks in an LDS slot, the lane walk or the
// code-by-code walk into an LDS output slot, then the store plan) and the global walk (persist_literal); the
// kernel's loop chooses between them (hpk_persist.h, "staged or global"). Plain per-lane code on hpk_walk.h and hpk_huge_piece.h alone: the including file
// provides the HIP runtime, u32x4 and hpk_bswap32 (hpk_persist.h through hpk_decode_kernel.h), or tests/emu/shim.h
// when tests/emu/persist_emu.cpp replays these functions on the CPU against the oracle.
#pragma once
#include "hpk_walk.h"
#include "hpk_huge_piece.h"

namespace hpkdec {

// The request's pointers come from memory, not from kernel arguments, so the compiler cannot tell they are
// global and would use flat accesses, which count in lgkmcnt too: every LDS lookup of the walk then waited
// for the output stores in flight (~27 us for one 27-byte literal per lane). Global address space, explicitly.
#ifndef HPK_GAS
#define HPK_GAS __attribute__((address_space(1)))
#endif

// One literal: huffman.rs:95-161 semantics (a code that runs past the end ends the walk, EOS is
// EOSInString at once, then > 7 residual bits PaddingTooLarge, non-ones InvalidPadding), and the batch
// ABI's capacity check per byte (HPK_OUTPUT_OVERFLOW, as the fill kernels' byte path:
// hpk_walk.h lit_bytes_to). Returns false (nothing written) if the literal's offsets are bad.
template <class Ld>
__device__ bool persist_literal(const Ld& ld16, const uint32_t* __restrict__ lut, const uint16_t* __restrict__ lo,
                                HPK_GAS uint8_t* out_base, uint32_t out_mis, uint32_t in_mis, uint32_t p0, uint32_t p1,
                                uint32_t o0, uint32_t o1, uint32_t& cnt, uint32_t& st) {
    const uint32_t nbits = (p1 - p0) * 8u, cap = o1 - o0;
    const uint32_t ob = out_mis + o0;  // (out_base-relative)
    cnt = 0;
    st = HPK_OK;
    if (nbits == 0u) return true;
    HugeWalk W;
    huge_begin(W, ld16, p0 + in_mis, 0u);
    uint64_t acc = 0;  // pending bytes of the 8-byte group holding position ob + cnt
    auto emit = [&](uint32_t sym) {
        const uint32_t p = ob + cnt;
        acc |= (uint64_t)sym << (8u * (p & 7u));
        if ((p & 7u) == 7u) {  // a group is complete: 8 bytes at once, or its bytes from ob on
            const uint32_t g = p - 7u;
            if (g >= ob)
                *(HPK_GAS uint64_t*)(out_base + g) = acc;
            else
                for (uint32_t x = ob; x <= p; ++x) out_base[x] = (uint8_t)(acc >> (8u * (x & 7u)));
            acc = 0;
        }
        cnt += 1u;
    };
    while (W.pos < nbits) {
        uint32_t sym, len, sym1, held;
        bool eos;
        huge_peek<3>(W, ld16, lut, lo, sym, len, eos, sym1, held);
        const uint32_t rem = nbits - W.pos;
        if (held != 0u && held <= rem && cnt + 2u <= cap) {  // two codes of <= 12 bits, both inside
            emit(sym);
            emit(sym1);
            huge_adv(W, held);
            continue;
        }
        if (len > rem) {  // huffman.rs:128-160
            st = residual_status(rem, (uint32_t)(W.win >> 32));
            break;
        }
        if (eos) {  // huffman.rs:112-116
            st = HPK_EOS_IN_STRING;
            break;
        }
        if (cnt >= cap) {
            st = HPK_OUTPUT_OVERFLOW;
            break;
        }
        emit(sym);
        huge_adv(W, len);
    }
    const uint32_t pe = ob + cnt;  // the last partial group, bytewise
    for (uint32_t x = max(ob, pe & ~7u); x < pe; ++x) out_base[x] = (uint8_t)(acc >> (8u * (x & 7u)));
    return true;
}

// The same walk over the literal staged in LDS: its 16-byte chunks loaded at once (one memory latency
// instead of one per chunk crossing: the global walker above took ~30 us for a 27-byte literal), stored
// big-endian into the lane's slot (dword j of lane t at slot[j * kThreads + t]: no bank conflicts).
constexpr uint32_t kPersistSlotChunks = 8;  // 128 bytes per lane: literals of <= 113 bytes (else the global walk)
constexpr uint32_t kPersistSlotMax = 113;   // (their decoded bound, 180 bytes, fits the output slot)

// Output: the walk writes the literal's bytes into the lane's LDS output slot, at the byte's position on
// the global 4-byte grid (slot byte (ob & 3) + k), and they leave it after the walk: the head's bytes up
// to the first 4-aligned address, then every whole dword, then the tail's bytes, the stores unrolled with
// their own registers. (Stores inside the walk made it wait for each one to complete before the next
// group's register could be written: ~25 us for a 27-byte literal.)
constexpr uint32_t kPersistOutDw = 48;  // output slot dwords per lane: 113 bytes decode to <= 180, + 3 of alignment, + 4
                                        // of a body step's garbage; the last byte is the checked steps' dummy

// Input slot: the lane's chunks as contiguous big-endian dwords after one pad dword (the lane walk reads
// dword (X >> 5) - 1), lane t's at slot + t * kPersistInStride: an odd stride, so the lanes' reads of the
// same dword fall in different banks.
// The lane walk reads dwords (X >> 5) + 1 and + 2 ahead of its position, so where a literal ends in its eighth
// chunk's last bytes it reads up to three dwords past its slot: the next lane's first dwords (behind the last
// lane's slot, what follows s_slot in LDS). They hold only bits past the literal's end, which decide nothing
// (hpk_walk.h); tests/emu/persist_emu.cpp varies them.
constexpr uint32_t kPersistInStride = 4u * kPersistSlotChunks + 1u;

template <int kThreads>
__device__ void persist_literal_lds(const HPK_GAS u32x4* __restrict__ g16, uint32_t last16, uint32_t* __restrict__ win32,
                                    uint8_t* __restrict__ oslot, const uint32_t* __restrict__ lut,
                                    const uint16_t* __restrict__ lo, HPK_GAS uint8_t* out_base, uint32_t out_mis,
                                    uint32_t in_mis, uint32_t p0, uint32_t p1, uint32_t o0, uint32_t o1, uint32_t& cnt,
                                    uint32_t& st, uint64_t* tl = nullptr) {
    const uint32_t nbytes = p1 - p0, b0 = p0 + in_mis, nbits = nbytes * 8u, cap = o1 - o0;
    const uint32_t c0 = b0 >> 4, nch = ((b0 + nbytes + 15u) >> 4) - c0;  // (<= kPersistSlotChunks)
    const uint32_t ob = out_mis + o0;
    const uint32_t oa = ob & 3u;  // the output slot's first byte sits at its global address mod 4
    cnt = 0;
    st = HPK_OK;
    if (nbits == 0u) return;
    u32x4 v[kPersistSlotChunks];
#pragma unroll
    for (uint32_t j = 0; j < kPersistSlotChunks; ++j) v[j] = j < nch ? g16[min(c0 + j, last16)] : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t j = 0; j < kPersistSlotChunks; ++j) {
        win32[1u + 4u * j] = hpk_bswap32(v[j].x);
        win32[2u + 4u * j] = hpk_bswap32(v[j].y);
        win32[3u + 4u * j] = hpk_bswap32(v[j].z);
        win32[4u + 4u * j] = hpk_bswap32(v[j].w);
    }
    if (tl) tl[1] = __builtin_amdgcn_s_memtime();
    const uint32_t sb = 32u + (b0 & 15u) * 8u;  // the literal's first bit in the window
    if (cap >= (nbytes * 8u) / 5u) {
        // a region that holds the decoded bound: the wave kernel's lane walk (body steps while >= kBodyMin
        // bits are left, then checked steps), bytes into the output slot, unconditional stores (kPred:
        // the dummy byte at kPersistOutDw * 4 - 1)
        Lit12 L;
        L.X = sb + 31u;
        L.Eb = L.X + nbits;
        L.o = oa;
        L.o0 = oa;
        L.oend = 0;
        L.st = HPK_OK;
        L.more = true;
        lit12_load(L, win32);
        bool body = L.Eb - L.X >= kBodyMin;
        while (body) lit12_body<kPred, 3>(L, win32, lut, lo, oslot, body);
        while (L.more) lit12_step<kPred, false, 3, true>(L, win32, lut, lo, oslot, kPersistOutDw * 4u - 1u);
        cnt = L.o - L.o0;
        st = lit12_status(L);
    } else {
        // a region below the decoded bound: code by code, the capacity checked per byte (the fill kernels'
        // byte path, hpk_decode_kernel.h lit_bytes_to)
        uint32_t q = sb >> 5;
        uint64_t win = ((uint64_t)win32[q] << 32) << (sb & 31u);
        uint32_t nb = 32u - (sb & 31u), pos = 0;
        q += 1u;
        while (pos < nbits) {
            if (nb <= 32u) {  // (q stays inside the slot: past the literal's chunks it reads zeros)
                win |= (uint64_t)win32[min(q, 4u * kPersistSlotChunks)] << (32u - nb);
                nb += 32u;
                q += 1u;
            }
            const uint32_t w = (uint32_t)(win >> 32);
            uint32_t sym, len;
            bool eos;
            lo_decode(w, lo, sym, len, eos);
            const uint32_t rem = nbits - pos;
            if (len > rem) {  // huffman.rs:128-160
                st = residual_status(rem, w);
                break;
            }
            if (eos) {  // huffman.rs:112-116
                st = HPK_EOS_IN_STRING;
                break;
            }
            if (cnt >= cap) {
                st = HPK_OUTPUT_OVERFLOW;
                break;
            }
            oslot[oa + cnt] = (uint8_t)sym;
            cnt += 1u;
            win <<= len;
            nb -= len;
            pos += len;
        }
    }
    if (tl) tl[2] = __builtin_amdgcn_s_memtime();
    // [ob, ob + cnt): head bytes up to the 4-aligned address h, whole dwords [h, t), tail bytes [t, ob + cnt)
    const uint32_t e = ob + cnt, h = min((ob + 3u) & ~3u, e), t = max(e & ~3u, h);
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k)
        if (ob + k < h) out_base[ob + k] = oslot[oa + k];
    // the dwords: those before the first 16-aligned address h16 and from the last one t16 on singly, the
    // 16-byte groups between as 16-byte stores (a store instruction per group, not per dword)
    const uint32_t* const os32 = reinterpret_cast<const uint32_t*>(oslot);
    const uint32_t base = ob - oa;  // the slot's first byte's address (4-aligned)
    const uint32_t h16 = min((h + 15u) & ~15u, t), t16 = max(t & ~15u, h16);
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k)
        if (h + 4u * k < h16) *reinterpret_cast<HPK_GAS uint32_t*>(out_base + h + 4u * k) = os32[(h - base) / 4u + k];
#pragma unroll
    for (uint32_t k = 0; k < kPersistOutDw / 4u; ++k)
        if (h16 + 16u * k < t16) {
            const uint32_t d = (h16 - base) / 4u + 4u * k;
            *reinterpret_cast<HPK_GAS u32x4*>(out_base + h16 + 16u * k) = u32x4{os32[d], os32[d + 1u], os32[d + 2u], os32[d + 3u]};
        }
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k)
        if (t16 + 4u * k < t) *reinterpret_cast<HPK_GAS uint32_t*>(out_base + t16 + 4u * k) = os32[(t16 - base) / 4u + k];
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k)
        if (t + k < e) out_base[t + k] = oslot[t + k - (ob - oa)];
    if (tl) tl[3] = __builtin_amdgcn_s_memtime();
}

}  // namespace hpkdec
