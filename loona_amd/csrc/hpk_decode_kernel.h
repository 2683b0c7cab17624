// hpk_decode_kernel.h — what the gfx950 decode kernels (hpk_wave.h, hpk_fill.h, hpk_persist.h and the
// phases hpk_long.h, hpk_huge.h; design notes in hpk_decode.hip) share beyond the lane walk
// (hpk_walk.h): kernel arguments, the table carve-out in LDS, the longest-first bucket, the
// LDS-only barrier. Earlier kernels built on them (v3-v11) are in git history (bench/legacy_decode*.h
// until round 3).
#pragma once
#include <stdint.h>

#include "hpk_device.h"
#include "hpk_walk.h"

namespace hpkdec {

// Tables in LDS (once per workgroup): the leading-ones table LO (1.9 KiB, any code), in the workgroup-fill
// kernel behind 256 bytes that once held T8 (symbols of the <= 8-bit codes; nothing reads them, and that
// kernel's LDS layout is left as it is; the wave kernel has no such carve-out). 16-byte aligned.
constexpr int kT8Bytes = 256;
constexpr int kLoBytes = HPK_LO_SIZE * 2;
constexpr int kTabBytes = ((kT8Bytes + kLoBytes + 15) / 16) * 16;

struct DecodeArgs {
    const uint8_t* in_base;  // in_blob rounded down to 16 bytes
    uint32_t in_mis;         // in_blob - in_base (0..15)
    const uint32_t* in_off;
    uint32_t n;
    uint8_t* out_base;  // out_blob rounded down to 16 bytes
    uint32_t out_mis;   // out_blob - out_base (0..15)
    const uint32_t* out_off;
    uint32_t* out_len;
    uint8_t* status;
    const uint16_t* lo;
    const uint32_t* lut2;   // two-symbol table (hpk_code.h) in the LUT2 layout (decode v12, the workgroup-fill kernel)
    const uint32_t* lut3;   // the same in the LUT3 layout (decode v28)
    const uint32_t* lut13;  // the LUT3 layout at 13 index bits (decode v39: the wave kernel, its long and huge phases)
    unsigned long long* dbg;  // diagnostic builds only: per-wave timestamps
    uint32_t in_cap, out_cap;  // blob sizes (clamped to HPK_MAX_OFFSET): larger offsets are bad
    uint32_t* err;             // sticky error flag (host-mapped): set to 1 on bad offsets
    // kLongK: literals of >= long_min encoded bytes (region >= the decoded bound) are left to the
    // long-literal phase (hpk_long.h): fill workgroup g lists them in long_list[its literal range),
    // those of >= long_big bytes from the front, the others from the back
    uint32_t* long_list;
    uint32_t long_min, long_big;
    // where the long- and huge-literal phases write literal i: lit_out[i] (out_off; in the compacted
    // mode the compacted offsets co_off, allocated when the literal is listed)
    const uint32_t* lit_out;
    // compacted mode (hpk_decode_batch_compact): co_off[i] = where literal i's bytes went, allocated from
    // the device cursor *cursor per fill (fill literals) or per listed literal (its decoded bound)
    uint32_t* co_off;
    uint32_t* cursor;
};

// Huge literals (hpk_huge.h) listed per workgroup in LDS; more go to the long-literal phase.
constexpr uint32_t kHugeMax = 16;

// a dword and four dwords stored at any byte address (unaligned global stores: the compacted forms)
typedef uint32_t u32u __attribute__((aligned(1)));
typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(1)));

// (compacted forms) length/status mark of a literal listed for a later phase, not decoded by its fill
constexpr uint32_t kListed = 0xFFFFFFFFu;

constexpr uint32_t kQ7Byte = 0x80000000u;  // queue entry .y flag: byte path

// Longest-first bucket of an encoded length (0 = longest): 2-byte classes up to 94 B, then
// 128-byte classes.
__device__ __forceinline__ uint32_t lpt_bucket(uint32_t nbytes) {
    const uint32_t b = nbytes < 96u ? (nbytes >> 1) : min(63u, 48u + ((nbytes - 96u) >> 7));
    return 63u - b;
}

// Workgroup barrier that orders LDS only: outstanding global stores (the previous fill's
// write-back) and prefetch loads stay in flight across it. __syncthreads() would wait for them.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

}  // namespace hpkdec
