// hpk_pack.h — the per-thread code of the ordered pack kernel (hpk_pack.hip): literal i's bytes
// src[src_off[i] .. src_off[i] + len[i]) laid end to end at dst[dst_off[i] ..), dst_off the exclusive
// sum of the lengths, as the reference's exact-length Vecs concatenated (huffman.rs:98, 160).
//
// The kernel is destination-centric: a thread makes one aligned 16-byte destination chunk at a time.
// It finds the chunk's first literal by binary search in the staged destination offsets, walks forward
// over however many literals the chunk spans (empty ones skipped), and takes each literal's share from
// the aligned source dwords that hold it, shifted into place by alignbit. Nothing here touches LDS
// or global memory except through the pointers it is given, so tests/emu/pack_emu.cpp runs these
// functions as they are on the host. pack2_chunk is pack_chunk with one of two source blobs per literal
// (hpk_pack2 in hpk_decode_strings.hip; tests/emu/pack2_emu.cpp).
#pragma once
#include <stdint.h>

#ifndef HPK_LDS_AS
#define HPK_LDS_AS __attribute__((address_space(3)))
#endif

namespace hpkpack {

// geometry (hpk_test_pack_geometry): a workgroup of kPackThreads threads makes destination tiles of
// kPackTile bytes, one 16-byte chunk per thread, from up to kPackLds literals' offsets staged in LDS
constexpr uint32_t kPackThreads = 256, kPackTile = kPackThreads * 16u, kPackLds = 2048;

// the source blob: its 16-byte-aligned base, its misalignment and its capacity (source offset x is byte
// mis + x from base); no dword outside the ones that hold [mis, mis + cap) is ever read
struct PackSrc {
    const uint32_t* base;
    uint32_t mis;
    uint32_t cap;
};

// how many of d[0 .. m) are <= x (d non-decreasing)
template <class DP>
__device__ __forceinline__ uint32_t pack_upper(DP d, uint32_t m, uint32_t x) {
    uint32_t lo = 0, hi = m;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (d[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ORs into acc (the chunk's four dwords) the bytes at chunk positions [q0, q1), 0 <= q0 < q1 <= 16:
// source offsets sa, sa + 1, ... (all below s.cap). The five aligned dwords around them are loaded
// only where they hold a wanted byte.
__device__ __forceinline__ void pack_segment(uint32_t acc[4], uint32_t q0, uint32_t q1, uint32_t sa, const PackSrc& s) {
    const uint32_t x0 = s.mis + sa, x1 = x0 + (q1 - q0) - 1u;  // first and last byte, from the aligned base
    const uint32_t xe = s.mis + s.cap - 1u;
    const uint32_t dlo = x0 >> 2, dhi = (x1 < xe ? x1 : xe) >> 2;
    const uint32_t z = x0 + 16u - q0;  // chunk position 0's byte, + 16 (it may lie before the base)
    const uint32_t r8 = (z & 3u) * 8u, dz = (z >> 2) - 4u;  // (dz wraps below 0: such dwords fail the range test)
    uint32_t w[5];
#pragma unroll
    for (uint32_t j = 0; j < 5u; ++j) {
        const uint32_t idx = dz + j;
        w[j] = (idx >= dlo && idx <= dhi) ? s.base[idx] : 0u;
    }
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t b0 = q0 > 4u * j ? q0 - 4u * j : 0u;
        const uint32_t b1 = q1 >= 4u * j + 4u ? 4u : (q1 > 4u * j ? q1 - 4u * j : 0u);
        if (b0 < b1) {
            const uint32_t mask = (0xFFFFFFFFu >> (8u * (4u - b1))) & (0xFFFFFFFFu << (8u * b0));
            acc[j] |= __builtin_amdgcn_alignbit(w[j + 1], w[j], r8) & mask;
        }
    }
}

// ORs into acc the bytes of destination offsets [lo, hi), lo < hi <= lo + 16, at chunk positions
// cpos, cpos + 1, ... (cpos + hi - lo <= 16). d[0 .. cnt] are the destination offsets of cnt staged
// literals and their end, so[0 .. cnt) their source offsets; d[0] <= lo and hi <= d[cnt].
// (One literal at a time: collecting up to four literals' shares first and issuing their loads
// together was slower, DESIGN.md §4.1e: the kernel is bound by instruction issue, not by load latency.)
template <class DP, class SP>
__device__ __forceinline__ void pack_chunk(uint32_t acc[4], DP d, SP so, uint32_t cnt, uint32_t lo, uint32_t hi,
                                           uint32_t cpos, const PackSrc& s) {
    uint32_t k = pack_upper(d, cnt + 1u, lo) - 1u;  // d[k] <= lo < d[k + 1]
    uint32_t o = lo;
    while (o < hi && k < cnt) {
        const uint32_t nx = d[k + 1u];
        if (nx <= o) {  // an empty literal
            ++k;
            continue;
        }
        const uint32_t e = nx < hi ? nx : hi;
        pack_segment(acc, cpos + (o - lo), cpos + (e - lo), so[k] + (o - d[k]), s);
        o = e;
    }
}

// pack_chunk with a source per literal (the string-literal decode's last step, hpk_decode_strings.hip): staged
// literal k's bytes are taken from s1 where sel[k] is nonzero, else from s0; so[k] is its offset in that
// source. Everything else as pack_chunk, so a chunk may mix bytes of both sources.
template <class DP, class SP, class XP>
__device__ __forceinline__ void pack2_chunk(uint32_t acc[4], DP d, SP so, XP sel, uint32_t cnt, uint32_t lo, uint32_t hi,
                                            uint32_t cpos, const PackSrc& s0, const PackSrc& s1) {
    uint32_t k = pack_upper(d, cnt + 1u, lo) - 1u;  // d[k] <= lo < d[k + 1]
    uint32_t o = lo;
    while (o < hi && k < cnt) {
        const uint32_t nx = d[k + 1u];
        if (nx <= o) {  // an empty literal
            ++k;
            continue;
        }
        const uint32_t e = nx < hi ? nx : hi;
        pack_segment(acc, cpos + (o - lo), cpos + (e - lo), so[k] + (o - d[k]), sel[k] ? s1 : s0);
        o = e;
    }
}

// A tile's chunk: chunk `c` of the tile whose first byte is destination coordinate t0 (coordinates
// count from the destination's 16-byte-aligned base, so the blob's offset x is coordinate mis + x).
// Offsets [*lo, *hi) are the chunk's share of [mis, end); false when it has none.
__device__ __forceinline__ bool pack_chunk_range(uint64_t t0, uint32_t c, uint32_t mis, uint64_t end, uint32_t* lo,
                                                 uint32_t* hi) {
    const uint64_t a0 = t0 + 16u * (uint64_t)c, a1 = a0 + 16u;
    const uint64_t b0 = a0 > mis ? a0 : mis, b1 = a1 < end ? a1 : end;
    if (b0 >= b1) return false;
    *lo = (uint32_t)(b0 - mis);
    *hi = (uint32_t)(b1 - mis);
    return true;
}

// writes the chunk: whole as one 16-byte store, a partial one (at the blob's misaligned start, at its
// end or at the capacity) byte by byte. p is the chunk's (16-byte-aligned) address.
__device__ __forceinline__ void pack_store(uint8_t* p, const uint32_t acc[4], uint32_t cpos, uint32_t nbytes) {
    if (nbytes == 16u) {
        uint4 v;  // (a nontemporal store here changed nothing)
        v.x = acc[0]; v.y = acc[1]; v.z = acc[2]; v.w = acc[3];
        *reinterpret_cast<uint4*>(p) = v;
        return;
    }
    for (uint32_t q = cpos; q < cpos + nbytes; ++q) p[q] = (uint8_t)(acc[q >> 2] >> (8u * (q & 3u)));
}

}  // namespace hpkpack
