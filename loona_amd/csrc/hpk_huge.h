// hpk_huge.h — huge-literal phase (decode v29): a literal of >= HPK_HUGE_MIN encoded bytes is decoded
// by up to a whole workgroup at once, in pieces, instead of by one lane of the long-literal phase.
//
// Why: one lane walks ~20 bits per ~600 cycles, so the long-literal phase took 125 ms for a 1 MiB
// literal where one CPU thread of the reference takes a few ms. Huffman codes do
// not mark their boundaries, so a piece that starts in the middle of a literal does not know where
// its first code starts; the walk is speculative and checked afterwards:
//   1. count: piece k of P (PB bytes each) walks from OV bits before its start (a code boundary
//      only by luck) to the first code that starts at or after its start (S_k), then counts the codes
//      that start in [S_k, start of piece k + 1) and stops at the first one that starts at or after
//      that (E_k). A walk resynchronises with the true one within a few dozen bits on header text
//      (scripts/sync_stats.py: 95 % within 128 bits), so S_k is the true boundary almost always.
//      Piece 0 starts at bit 0 (exact); the last piece walks to the literal's end;
//   2. fix: piece k is right iff S_k == E_{k-1} (its predecessor right). A piece that does not match
//      walks again from E_{k-1} (no lead); repeated until no piece changes (each round fixes at least
//      the first mismatch for good, and mismatches are rare and isolated);
//   3. the first piece that ends the walk — a code that does not fit (the literal's end, or
//      PaddingTooLarge), EOS — is the literal's last (t); pieces after it are ignored;
//   4. a scan of the counts of pieces 0..t gives each piece its output offset, and the pieces walk
//      again from S_k and store their codes (8-byte stores of whole groups, the two partial groups at a
//      piece's ends bytewise); piece t stores the length and status.
// Several huge literals share a round (a contiguous run of lanes each); rounds repeat until the
// workgroup's list is done. Input is read straight from global memory, 16-byte chunks one ahead of
// the walk. Semantics are the lane walk's (huffman.rs:95-161): a code that runs past the end stops the
// walk, EOS is EOSInString at once, then > 7 residual bits PaddingTooLarge, non-ones InvalidPadding.
// The per-piece functions are plain per-lane code in hpk_huge_piece.h (tests/emu replays them on the CPU).
#pragma once
#include "hpk_decode_kernel.h"
#include "hpk_huge_piece.h"

namespace hpkdec {

// The phase: all kBlock threads of the workgroup call it (after the fills, before the long-literal
// phase), with the workgroup's list s_list[0, cnt) of huge literals (validated when listed: offsets in
// bounds, regions >= the decoded bound) and a scratch area of LDS (kHugeLds bytes, 16-byte aligned).
template <int kBlock>
constexpr int huge_lds_bytes() {
    return 3 * kBlock * 4 + (5 * kHugeMax + 4 + 16) * 4;
}

template <int kBlock, int kTab>
__device__ void huge_phase(const DecodeArgs& a, const uint32_t* s_list, uint32_t cnt, uint32_t* meta,
                           const uint32_t* __restrict__ s_lut, const uint16_t* __restrict__ s_lo) {
    if (cnt == 0) return;  // (block-uniform)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t* const mE = meta;               // per piece: E and flag (read by the next piece), scan
    uint32_t* const mF = meta + kBlock;
    uint32_t* const mX = meta + 2 * kBlock;
    uint32_t* const jl = meta + 3 * kBlock;  // jobs: literal, first lane, pieces, terminal piece
    uint32_t* const jb = jl + kHugeMax;
    uint32_t* const jp = jb + kHugeMax;
    uint32_t* const jt = jp + kHugeMax;
    uint32_t* const jo = jt + kHugeMax;      // output offset (out_base-relative, before out_mis)
    uint32_t* const jm = jo + kHugeMax;      // [0] jobs, [1] next list entry, [2] lanes used, [3..4] fix flags
    uint32_t* const wt = jm + 4;             // wave totals of the scan
    const uint32_t in_end = min(a.in_off[a.n], a.in_cap) + a.in_mis;
    const uint32_t last16 = in_end ? (in_end - 1u) >> 4 : 0u;
    const uint4* const g16 = reinterpret_cast<const uint4*>(a.in_base);
    auto ld16 = [&](uint32_t ci) { return g16[min(ci, last16)]; };
    uint8_t* const out = a.out_base;
    auto st8 = [&](uint32_t g, uint64_t v) { *reinterpret_cast<uint64_t*>(out + g) = v; };
    auto st1 = [&](uint32_t x, uint8_t v) { out[x] = v; };
    for (uint32_t cur = 0; cur < cnt;) {  // block-uniform
        __syncthreads();
        if (tid == 0) {  // the round's jobs: literals from the list while their pieces fit the block
            uint32_t nj = 0, used = 0, e = cur;
            for (; e < cnt && nj < kHugeMax; ++e) {
                const uint32_t i = s_list[e];
                const uint32_t nb = a.in_off[i + 1] - a.in_off[i];
                uint32_t P, PB, OV;
                huge_geometry(nb, kBlock, P, PB, OV);
                if (used + P > (uint32_t)kBlock) break;
                jl[nj] = i;
                // (the compacted mode, a.cursor set: the literal's decoded bound from the cursor, now)
                jo[nj] = a.cursor ? atomicAdd(a.cursor, (nb * 8u) / 5u) : a.lit_out[i];
                if (a.cursor) a.co_off[i] = jo[nj];
                jb[nj] = used;
                jp[nj] = P;
                jt[nj] = kHugeNone;
                used += P;
                ++nj;
            }
            jm[0] = nj;
            jm[1] = e;
            jm[2] = used;
            jm[3] = 0;
        }
        __syncthreads();
        const uint32_t nj = jm[0], used = jm[2];
        cur = jm[1];
        const bool on = tid < used;
        uint32_t j = 0;
        for (uint32_t q = 1; q < nj; ++q) j = jb[q] <= tid ? q : j;
        const uint32_t i = jl[j], base = jb[j], obase = jo[j];
        const uint32_t k = tid - base;
        const uint32_t p0 = a.in_off[i], nbytes = a.in_off[i + 1] - p0;
        const uint32_t lbyte = p0 + a.in_mis;
        uint32_t P, PB, OV;
        huge_geometry(nbytes, kBlock, P, PB, OV);
        uint32_t S = 0, E = 0, c = 0, fl = 0;
        if (on) {
            huge_pass1<kTab>(ld16, s_lut, s_lo, lbyte, nbytes, k, P, PB, OV, S, E, c, fl);
            mE[tid] = E;
            mF[tid] = fl;
        }
        // the fix rounds: "any piece re-walks" through a pair of LDS flags (round r sets flag r % 2 and
        // clears the other, which every thread has read before this round's first barrier)
        for (uint32_t r = 0;; ++r) {
            __syncthreads();
            bool need = false;
            uint32_t from = 0;
            if (on && k > 0u) {
                const uint32_t pe = mE[tid - 1], pf = mF[tid - 1];
                need = !(pf & kHugeTerm) && pe != kHugeNone && S != pe;
                from = pe;
            }
            if (tid == 0) jm[3 + ((r + 1u) & 1u)] = 0;
            if (need) jm[3 + (r & 1u)] = 1;
            __syncthreads();
            if (jm[3 + (r & 1u)] == 0u) break;
            if (need) {
                huge_refix<kTab>(ld16, s_lut, s_lo, lbyte, nbytes, k, P, PB, from, S, E, c, fl);
                mE[tid] = E;
                mF[tid] = fl;
            }
        }
        if (on && (fl & kHugeTerm)) atomicMin(&jt[j], k);
        __syncthreads();
        const uint32_t t = on ? jt[j] : 0u;
        const bool live = on && k <= t;
        // exclusive scan of the live pieces' counts over the block
        const uint32_t v = live ? c : 0u;
        uint32_t x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d);
            if (lane >= (uint32_t)d) x += y;
        }
        if (lane == 63u) wt[wv] = x;
        __syncthreads();
        uint32_t pre = 0;
        for (uint32_t q = 0; q < wv; ++q) pre += wt[q];
        const uint32_t ex = pre + x - v;
        mX[tid] = ex;
        __syncthreads();
        if (live) {
            const uint32_t D = ex - mX[base];
            huge_pass2<kTab>(ld16, s_lut, s_lo, lbyte, S, c, obase + a.out_mis + D, st8, st1);
            if (k == t) {
                a.out_len[i] = D + c;
                a.status[i] = (uint8_t)(fl & 0xFFu);
            }
        }
    }
    __syncthreads();
}

}  // namespace hpkdec
