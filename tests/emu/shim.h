// host emulation shim for the per-lane headers of loona_amd/csrc (hpk_walk.h, hpk_huge_piece.h), included
// before them: what they use of the HIP language and builtins, one lane at a time
#pragma once
#include <stdint.h>
#include <algorithm>
#define __device__
#define __forceinline__ inline
#define __restrict__
#define HPK_LDS_AS
using std::min; using std::max;
static inline uint32_t __builtin_amdgcn_alignbit(uint32_t a, uint32_t b, uint32_t s) {
    return (uint32_t)((((uint64_t)a << 32) | b) >> (s & 31));
}
static inline uint32_t __clz(uint32_t x){ return x? __builtin_clz(x):32; }
struct uint4 { uint32_t x, y, z, w; };
// hpk_persist_lit.h: global pointers are plain ones, the 4-dword vector, the byte swap, the shader clock
#define HPK_GAS
struct u32x4 { uint32_t x, y, z, w; };
static inline uint32_t hpk_bswap32(uint32_t x) { return __builtin_bswap32(x); }
static inline uint64_t __builtin_amdgcn_s_memtime() { return 0; }
