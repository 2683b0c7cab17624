// hpk_frmwrite.h — the per-thread code of the frame write (hpk_frmwrite.hip): header block b, the bytes
// src[block_off[b] .. block_off[b+1]) of length L, becomes one HEADERS frame and as many CONTINUATION frames as
// its peer's SETTINGS_MAX_FRAME_SIZE M demands, laid at dst[wire_off[b] ..): the reference's loop in
// send_data_maybe (crates/loona/src/h2/server.rs:470-508: a piece strictly longer than M goes as M octets with
// no flag, the last piece of 1..M octets, or of 0 for the empty block, carries END_HEADERS) with
// Frame::write_into's header (crates/loona-h2/src/lib.rs:413-422) in front of every piece.
//
// Every frame but the last takes M + 9 octets, so position p of a block's wire lies in frame f = p / (M + 9) at
// r = p % (M + 9): a header octet made in registers when r < 9, else source octet block_off[b] + f M + r - 9.
// The kernel is destination-centric like the ordered pack and shares its chunk code (hpk_pack.h): a thread makes
// one aligned 16-byte destination chunk at a time, finds the chunk's first block by binary search in the staged
// wire offsets and walks forward over the blocks the chunk spans (those of no octets skipped). A piece of a chunk
// that lies wholly inside one payload costs the one division and pack_segment's aligned loads; only a piece that
// touches a header goes octet by octet. Nothing here touches LDS or global memory except through the pointers it
// is given, so tests/emu/frmwrite_emu.cpp runs these functions as they are on the host.
#pragma once
#include <stdint.h>

#include "hpk_pack.h"

namespace hpkfw {
using hpkpack::PackSrc;

// geometry (hpk_test_frmwrite_geometry): a workgroup of kFwThreads threads makes destination tiles of kFwTile
// bytes, one 16-byte chunk per thread, from up to kFwLds blocks' offsets, frame sizes and stream words in LDS
constexpr uint32_t kFwThreads = 256, kFwTile = kFwThreads * 16u, kFwLds = 1024;
constexpr uint32_t kFwMaxFrame = 0xFFFFFFu;  // the length field has 24 bits

// whether block [a, e) with frame size m can be written: else it is void (0 octets, HPK_BAD_OFFSETS)
__device__ __forceinline__ bool fw_block_ok(uint32_t a, uint32_t e, uint32_t m, uint32_t cap) {
    return a <= e && e <= cap && m >= 1u && m <= kFwMaxFrame;
}

// max(1, ceil(L / m)), m >= 1: L = k m gives k frames, no empty CONTINUATION behind them
__device__ __forceinline__ uint32_t fw_frames(uint32_t L, uint32_t m) {
    const uint32_t q = L / m, f = q + (q * m != L ? 1u : 0u);
    return f ? f : 1u;
}

// a block's octets on the wire; 64 bits: L near 2^32 / 10 with m = 1 passes 32
__device__ __forceinline__ uint64_t fw_wire_len(uint32_t L, uint32_t m) { return (uint64_t)L + 9ull * fw_frames(L, m); }

// the length scan's element
__device__ __forceinline__ uint64_t fw_elem(uint32_t a, uint32_t e, uint32_t m, uint32_t cap) {
    return fw_block_ok(a, e, m, cap) ? fw_wire_len(e - a, m) : 0ull;
}

// octet r < 9 of frame f's header: the 24-bit length (M for every frame but the last, the rest for the last, 0
// for the empty block), the type (HEADERS 0x1, then CONTINUATION 0x9), the flags (END_HEADERS 0x4 on the last
// frame, END_STREAM 0x1 on the HEADERS frame when sid's bit 31 asks for it) and the 31-bit stream id
__device__ __forceinline__ uint32_t fw_header_octet(uint32_t r, uint32_t f, uint32_t L, uint32_t M, uint32_t sid) {
    const uint32_t rest = L - f * M;
    const bool last = rest <= M;
    const uint32_t len = last ? rest : M;
    const uint32_t flags = (last ? 4u : 0u) | ((f == 0u && (sid >> 31)) ? 1u : 0u);
    const uint32_t id = sid & 0x7FFFFFFFu;
    // octets 0..3 and 4..7 as little-endian words, octet 8 the id's lowest
    const uint32_t w0 = (len >> 16) | ((len >> 8 & 255u) << 8) | ((len & 255u) << 16) | ((f ? 9u : 1u) << 24);
    const uint32_t w1 = flags | ((id >> 24) << 8) | ((id >> 16 & 255u) << 16) | ((id >> 8 & 255u) << 24);
    const uint32_t w = r < 4u ? w0 : w1;
    return r < 8u ? (w >> (8u * (r & 3u))) & 255u : id & 255u;
}

// ORs octet v into chunk position q of acc (no dynamic register index)
__device__ __forceinline__ void fw_put(uint32_t acc[4], uint32_t q, uint32_t v) {
    const uint32_t x = v << (8u * (q & 3u)), d = q >> 2;
    acc[0] |= d == 0u ? x : 0u;
    acc[1] |= d == 1u ? x : 0u;
    acc[2] |= d == 2u ? x : 0u;
    acc[3] |= d == 3u ? x : 0u;
}

// ORs into acc, at chunk positions q0, q0 + 1, ..., the n octets (1 <= n, q0 + n <= 16) at positions p0 .. of the
// wire of the block [a, a + L) with frame size M and stream word sid; p0 + n <= fw_wire_len(L, M)
__device__ __forceinline__ void fw_piece(uint32_t acc[4], uint32_t q0, uint32_t p0, uint32_t n, uint32_t a, uint32_t L,
                                         uint32_t M, uint32_t sid, const PackSrc& s) {
    const uint32_t stride = M + 9u;
    uint32_t f = p0 / stride;
    uint32_t r = p0 - f * stride;
    if (r >= 9u && r + n <= stride) {  // wholly inside one payload: the common case
        hpkpack::pack_segment(acc, q0, q0 + n, a + f * M + (r - 9u), s);
        return;
    }
    uint32_t j = 0;
    while (j < n) {
        if (r < 9u) {
            fw_put(acc, q0 + j, fw_header_octet(r, f, L, M, sid));
            ++j;
            ++r;
        } else {
            const uint32_t left = n - j, room = stride - r;
            const uint32_t run = left < room ? left : room;
            hpkpack::pack_segment(acc, q0 + j, q0 + j + run, a + f * M + (r - 9u), s);
            j += run;
            r += run;
        }
        if (r == stride) {
            r = 0u;
            ++f;
        }
    }
}

// ORs into acc the octets of wire offsets [lo, hi), lo < hi <= lo + 16, at chunk positions cpos, cpos + 1, ...
// (cpos + hi - lo <= 16). wd[0 .. cnt] are the wire offsets of cnt staged blocks and their end, bo[0 .. cnt] their
// source offsets and the last one's end, mf[0 .. cnt) their frame sizes and sid[0 .. cnt) their stream words;
// wd[0] <= lo and hi <= wd[cnt]. A staged block of no octets (a void one) is skipped: nothing of it is trusted.
template <class WP, class BP, class MP, class SP>
__device__ __forceinline__ void fw_chunk(uint32_t acc[4], WP wd, BP bo, MP mf, SP sid, uint32_t cnt, uint32_t lo, uint32_t hi,
                                         uint32_t cpos, const PackSrc& s) {
    uint32_t k = hpkpack::pack_upper(wd, cnt + 1u, lo) - 1u;  // wd[k] <= lo < wd[k + 1]
    uint32_t o = lo;
    while (o < hi && k < cnt) {
        const uint32_t nx = wd[k + 1u];
        if (nx <= o) {  // a block of no octets
            ++k;
            continue;
        }
        const uint32_t e = nx < hi ? nx : hi;
        const uint32_t a = bo[k];
        fw_piece(acc, cpos + (o - lo), o - wd[k], e - o, a, bo[k + 1u] - a, mf[k], sid[k], s);
        o = e;
    }
}

}  // namespace hpkfw
