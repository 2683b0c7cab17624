// hpk_scan.h — the tiled exclusive scan of the batch calls: out[i] = the u32 sum of elements 0 .. i - 1,
// n + 1 entries, in three launches on one stream: per 4,096-element tile its sum, one workgroup scanning the
// tile sums in place, every tile scanned again from its base (reads an element's source twice and writes
// 4 B per element; hipcub's scan over a transform iterator took 151 us per 32M elements, round 5).
//
// Elem says what an element is. It is passed to the kernels by value and has
//   void tile(n, base, s, v): the thread's kK consecutive elements base + kK * threadIdx.x + k into v[k]
//       (0 at and past n), with s (kTile + 1 words of LDS) to stage the tile through;
//   tile_sum(n, base, s): the sum of kK of the tile's elements, every thread's its own (in the width it needs).
// Sum is the type of the tile sums. uint32_t: the offsets are sums mod 2^32. uint64_t: a total past
// HPK_MAX_OFFSET makes every output 0 and stores 1 to *err, so the output never wraps.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hpk.h"

namespace hpkscan {
constexpr uint32_t kT = 256, kK = 16, kTile = kT * kK;

__device__ __forceinline__ uint32_t shfl_up(uint32_t x, uint32_t d) { return (uint32_t)__shfl_up((int)x, d); }
__device__ __forceinline__ uint64_t shfl_up(uint64_t x, uint32_t d) {
    return ((uint64_t)shfl_up((uint32_t)(x >> 32), d) << 32) | shfl_up((uint32_t)x, d);
}

// exclusive block scan of one value per thread (kT threads), the total to *tot
template <class T>
__device__ __forceinline__ T block_exscan(T v, T* s_w, T* tot) {
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    T x = v;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const T y = shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63u) s_w[w] = x;
    __syncthreads();
    T pre = 0, all = 0;
#pragma unroll
    for (uint32_t q = 0; q < kT / 64u; ++q) {
        pre += q < w ? s_w[q] : (T)0;
        all += s_w[q];
    }
    *tot = all;
    return pre + x - v;
}

template <class Sum, class Elem>
__global__ __launch_bounds__(kT) void tile_sums(Elem e, uint32_t n, Sum* __restrict__ sums) {
    __shared__ uint32_t s[kTile + 1];
    __shared__ Sum s_w[kT / 64];
    Sum tot;
    (void)block_exscan<Sum>((Sum)e.tile_sum(n, blockIdx.x * kTile, s), s_w, &tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// one workgroup: the tile sums' exclusive scan, in place; 64-bit sums: sums[nt] = 1 when the total does not fit
template <class Sum>
__global__ __launch_bounds__(kT) void sums_scan(Sum* __restrict__ sums, uint32_t nt) {
    __shared__ Sum s_w[kT / 64];
    Sum carry = 0;
    for (uint32_t b0 = 0; b0 < nt; b0 += kTile) {
        const uint32_t t = threadIdx.x;
        Sum v[kK], acc = 0;
#pragma unroll
        for (uint32_t k = 0; k < kK; ++k) {
            const uint32_t j = b0 + t * kK + k;
            v[k] = j < nt ? sums[j] : (Sum)0;
            acc += v[k];
        }
        Sum tot;
        Sum x = carry + block_exscan<Sum>(acc, s_w, &tot);
#pragma unroll
        for (uint32_t k = 0; k < kK; ++k) {
            const uint32_t j = b0 + t * kK + k;
            if (j < nt) sums[j] = x;
            x += v[k];
        }
        carry += tot;
        __syncthreads();  // (s_w reused)
    }
    if constexpr (sizeof(Sum) == 8)
        if (threadIdx.x == 0) sums[nt] = carry > (uint64_t)HPK_MAX_OFFSET ? 1u : 0u;
}

template <class Sum, class Elem>
__global__ __launch_bounds__(kT) void tile_scan(Elem e, uint32_t n, const Sum* __restrict__ sums, uint32_t nt,
                                                uint32_t* __restrict__ out, uint32_t* __restrict__ err) {
    __shared__ uint32_t s[kTile + 1];
    __shared__ uint32_t s_w[kT / 64];
    const uint32_t base = blockIdx.x * kTile, t = threadIdx.x;
    if constexpr (sizeof(Sum) == 8) {
        if (sums[nt] != 0u) {  // the total passes u32 offsets
#pragma unroll
            for (uint32_t k = 0; k < kK; ++k) {
                const uint32_t j = base + t + kT * k;
                if (j <= n) out[j] = 0u;
            }
            if (t == 0) *err = 1u;
            return;
        }
    }
    uint32_t v[kK], acc = 0;
    e.tile(n, base, s, v);
#pragma unroll
    for (uint32_t k = 0; k < kK; ++k) acc += v[k];
    uint32_t tot;
    uint32_t x = (uint32_t)sums[blockIdx.x] + block_exscan<uint32_t>(acc, s_w, &tot);
    __syncthreads();  // (every thread's elements are read: the staged tile gives way to its results)
#pragma unroll
    for (uint32_t k = 0; k < kK; ++k) {
        s[t * kK + k] = x;
        x += v[k];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kK; ++k) {  // (striped, coalesced)
        const uint32_t j = base + t + kT * k;
        if (j <= n) out[j] = s[t + kT * k];
    }
}

inline uint32_t tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + 1u + kTile - 1u) / kTile); }  // over n + 1 elements

// the device scratch a scan of n elements needs
template <class Sum>
inline size_t tmp_bytes(uint32_t n) {
    return ((size_t)tiles(n) + (sizeof(Sum) == 8 ? 1u : 0u)) * sizeof(Sum);
}

template <class Sum, class Elem>
inline void launch(hipStream_t stream, Elem e, uint32_t n, uint32_t* out, void* tmp, uint32_t* err) {
    const uint32_t nt = tiles(n);
    Sum* sums = static_cast<Sum*>(tmp);
    hipLaunchKernelGGL((tile_sums<Sum, Elem>), dim3(nt), dim3(kT), 0, stream, e, n, sums);
    hipLaunchKernelGGL((sums_scan<Sum>), dim3(1), dim3(kT), 0, stream, sums, nt);
    hipLaunchKernelGGL((tile_scan<Sum, Elem>), dim3(nt), dim3(kT), 0, stream, e, n, (const Sum*)sums, nt, out, err);
}
}  // namespace hpkscan
