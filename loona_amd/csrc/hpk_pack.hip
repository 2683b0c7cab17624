// hpk_pack.hip — the ordered pack: literals held anywhere in a source blob laid end to end, in literal
// order, with no gap (hpk_decode_batch_packed's last step, and hpk_pack_batch on its own). The result is
// what the reference's exact-length Vecs (huffman.rs:98, 160) would be, concatenated.
//
// Two steps on the context's stream:
//   * the length scan: dst_off = the exclusive u32 sum of the n lengths (n + 1 entries), in three
//     launches like the compacted form's bound scan (hpk_decode.hip): per 4,096-element tile its sum,
//     one workgroup scanning the tile sums, every tile scanned again from its base. A literal that
//     passes the source capacity counts 0 bytes (and sets the sticky error flag); the tile sums are
//     64-bit, and a total past HPK_MAX_OFFSET makes every length count 0 (flag set), so dst_off is
//     always non-decreasing and the pack below never meets a wrapped offset;
//   * hpk_pack (per-thread code in hpk_pack.h): destination-centric. The destination, counted from its
//     16-byte-aligned base, is cut into tiles of kPackTile bytes; a workgroup takes a contiguous run of
//     tiles, finds its first literal by one binary search of dst_off, and from then on keeps a window
//     of up to kPackLds literals' dst_off / src_off in LDS, restaged when the tiles have used it up
//     (so each offset is read once per workgroup, and a tile that covers more literals than the window
//     holds is made in rounds). Each thread makes one aligned 16-byte chunk per tile and stores it
//     whole; the partial chunks at a misaligned start, at dst_off[n] and at the capacity go bytewise.
//     Bytes at or past min(dst_off[n], dst_cap) are never written.
#include "hpk_device.h"
#include "hpk_pack.h"

using namespace hpkpack;

namespace {
constexpr uint32_t kLenT = 256, kLenK = 16, kLenTile = kLenT * kLenK;

// literal i's length as the pack counts it: 0 when its bytes would pass the source capacity
__device__ __forceinline__ uint32_t len_of(uint32_t off, uint32_t len, uint32_t cap, bool* bad) {
    const bool ok = len == 0u || (off <= cap && len <= cap - off);
    *bad |= !ok;
    return ok ? len : 0u;
}

__device__ __forceinline__ uint64_t shfl_up64(uint64_t x, uint32_t d) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)x, d), hi = (uint32_t)__shfl_up((int)(uint32_t)(x >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}

// exclusive block scan of one value per thread (kLenT threads), the total to *tot
template <class T>
__device__ __forceinline__ T block_exscan(T v, T* s_w, T* tot) {
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    T x = v;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        T y;
        if constexpr (sizeof(T) == 8) y = shfl_up64(x, d); else y = (T)__shfl_up((int)x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63u) s_w[w] = x;
    __syncthreads();
    T pre = 0, all = 0;
#pragma unroll
    for (uint32_t q = 0; q < kLenT / 64u; ++q) {
        pre += q < w ? s_w[q] : (T)0;
        all += s_w[q];
    }
    *tot = all;
    return pre + x - v;
}

__global__ __launch_bounds__(kLenT) void pack_len_sums(const uint32_t* __restrict__ off, const uint32_t* __restrict__ len,
                                                       uint32_t n, uint32_t cap, uint64_t* __restrict__ sums) {
    __shared__ uint64_t s_w[kLenT / 64];
    const uint32_t base = blockIdx.x * kLenTile, t = threadIdx.x;
    uint32_t o[kLenK], l[kLenK];
#pragma unroll
    for (uint32_t k = 0; k < kLenK; ++k) {  // (all the loads first)
        const uint32_t j = base + t + kLenT * k;
        o[k] = j < n ? off[j] : 0u;
        l[k] = j < n ? len[j] : 0u;
    }
    uint64_t acc = 0;
    bool bad = false;
#pragma unroll
    for (uint32_t k = 0; k < kLenK; ++k) acc += len_of(o[k], l[k], cap, &bad);
    uint64_t tot;
    (void)block_exscan<uint64_t>(acc, s_w, &tot);
    if (t == 0) sums[blockIdx.x] = tot;
}

// one workgroup: the tile sums' exclusive scan, in place; sums[nt] = 1 when the total does not fit
__global__ __launch_bounds__(kLenT) void pack_sums_scan(uint64_t* __restrict__ sums, uint32_t nt) {
    __shared__ uint64_t s_w[kLenT / 64];
    uint64_t carry = 0;
    for (uint32_t b0 = 0; b0 < nt; b0 += kLenTile) {
        const uint32_t t = threadIdx.x;
        uint64_t v[kLenK], acc = 0;
#pragma unroll
        for (uint32_t k = 0; k < kLenK; ++k) {
            const uint32_t j = b0 + t * kLenK + k;
            v[k] = j < nt ? sums[j] : 0u;
            acc += v[k];
        }
        uint64_t tot;
        uint64_t x = carry + block_exscan<uint64_t>(acc, s_w, &tot);
#pragma unroll
        for (uint32_t k = 0; k < kLenK; ++k) {
            const uint32_t j = b0 + t * kLenK + k;
            if (j < nt) sums[j] = x;
            x += v[k];
        }
        carry += tot;
        __syncthreads();  // (s_w reused)
    }
    if (threadIdx.x == 0) sums[nt] = carry > (uint64_t)HPK_MAX_OFFSET ? 1u : 0u;
}

__global__ __launch_bounds__(kLenT) void pack_len_scan(const uint32_t* __restrict__ off, const uint32_t* __restrict__ len,
                                                       uint32_t n, uint32_t cap, const uint64_t* __restrict__ sums,
                                                       uint32_t nt, uint32_t* __restrict__ out, uint32_t* __restrict__ err) {
    __shared__ uint32_t s[kLenTile];
    __shared__ uint32_t s_w[kLenT / 64];
    const uint32_t base = blockIdx.x * kLenTile, t = threadIdx.x;
    if (sums[nt] != 0u) {  // the total passes u32 offsets: nothing is packed
#pragma unroll
        for (uint32_t k = 0; k < kLenK; ++k) {
            const uint32_t j = base + t + kLenT * k;
            if (j <= n) out[j] = 0u;
        }
        if (t == 0) *err = 1u;
        return;
    }
    uint32_t o[kLenK], l[kLenK];
#pragma unroll
    for (uint32_t k = 0; k < kLenK; ++k) {  // (striped, coalesced; all the loads first)
        const uint32_t j = base + t + kLenT * k;
        o[k] = j < n ? off[j] : 0u;
        l[k] = j < n ? len[j] : 0u;
    }
    bool bad = false;
#pragma unroll
    for (uint32_t k = 0; k < kLenK; ++k) s[t + kLenT * k] = len_of(o[k], l[k], cap, &bad);
    if (bad) *err = 1u;
    __syncthreads();
    uint32_t v[kLenK], acc = 0;
#pragma unroll
    for (uint32_t k = 0; k < kLenK; ++k) {
        v[k] = s[t * kLenK + k];
        acc += v[k];
    }
    uint32_t tot;
    uint32_t x = (uint32_t)sums[blockIdx.x] + block_exscan<uint32_t>(acc, s_w, &tot);
    __syncthreads();  // (every thread's lengths are read: they give way to the results)
#pragma unroll
    for (uint32_t k = 0; k < kLenK; ++k) {
        s[t * kLenK + k] = x;
        x += v[k];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kLenK; ++k) {
        const uint32_t j = base + t + kLenT * k;
        if (j <= n) out[j] = s[t + kLenT * k];
    }
}

struct PackArgs {
    PackSrc src;
    const uint32_t* src_off;
    const uint32_t* dst_off;
    uint32_t n;
    uint8_t* dst_base;  // 16-byte aligned: the blob starts dst_mis bytes in
    uint32_t dst_mis;
    uint32_t dst_cap;
};

constexpr uint32_t kPackLdsBytes = (2u * kPackLds + 4u) * 4u;

__global__ __launch_bounds__(kPackThreads) void hpk_pack(PackArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t pack_smem[];
    uint32_t* sd = pack_smem;                 // the window's dst_off, kPackLds + 1 entries
    uint32_t* ss = pack_smem + kPackLds + 4;  // its src_off
    const uint32_t tid = threadIdx.x, n = a.n;
    const uint32_t total = a.dst_off[n];
    const uint32_t limit = total < a.dst_cap ? total : a.dst_cap;
    if (limit == 0u) return;
    const uint64_t end = (uint64_t)a.dst_mis + limit;  // in coordinates from dst_base
    const uint64_t ntiles = (end + kPackTile - 1u) / kPackTile;
    const uint64_t per = (ntiles + gridDim.x - 1u) / gridDim.x;
    const uint64_t t_first = (uint64_t)blockIdx.x * per;
    const uint64_t t_last = t_first + per < ntiles ? t_first + per : ntiles;
    if (t_first >= t_last) return;
    const uint64_t c_first = t_first * kPackTile;
    // the literal that holds the run's first byte: dst_off[0] = 0 <= it < dst_off[n]
    uint32_t win_a = pack_upper(a.dst_off, n + 1u, (uint32_t)((c_first > a.dst_mis ? c_first : a.dst_mis) - a.dst_mis)) - 1u;
    uint32_t win_cnt = 0;  // literals [win_a, win_a + win_cnt) are staged; dst_off[win_a] <= cur throughout
    for (uint64_t t = t_first; t < t_last; ++t) {
        const uint64_t c0 = t * kPackTile, c1 = c0 + kPackTile;
        const uint32_t thi = (uint32_t)((c1 < end ? c1 : end) - a.dst_mis);
        uint32_t cur = (uint32_t)((c0 > a.dst_mis ? c0 : a.dst_mis) - a.dst_mis);
        uint32_t clo = 0, chi = 0;
        const bool have = pack_chunk_range(c0, tid, a.dst_mis, end, &clo, &chi);
        uint32_t acc[4] = {0u, 0u, 0u, 0u};
        while (cur < thi) {
            if (win_cnt == 0u || sd[win_cnt] <= cur) {  // (uniform) the window is used up: the next literals
                win_a += win_cnt;
                __syncthreads();
                win_cnt = n - win_a < kPackLds ? n - win_a : kPackLds;
                uint32_t vd[kPackLds / kPackThreads], vs[kPackLds / kPackThreads];
#pragma unroll
                for (uint32_t i = 0; i < kPackLds / kPackThreads; ++i) {  // (all the loads first)
                    const uint32_t j = tid + kPackThreads * i;
                    vd[i] = j < win_cnt ? a.dst_off[win_a + j] : 0u;
                    vs[i] = j < win_cnt ? a.src_off[win_a + j] : 0u;
                }
                if (tid == 0) sd[win_cnt] = a.dst_off[win_a + win_cnt];
#pragma unroll
                for (uint32_t i = 0; i < kPackLds / kPackThreads; ++i) {
                    const uint32_t j = tid + kPackThreads * i;
                    if (j < win_cnt) {
                        sd[j] = vd[i];
                        ss[j] = vs[i];
                    }
                }
                __syncthreads();
            }
            const uint32_t we = sd[win_cnt];
            const uint32_t rend = we < thi ? we : thi;  // this round: offsets [cur, rend)
            if (have) {
                const uint32_t lo = clo > cur ? clo : cur, hi = chi < rend ? chi : rend;
                if (lo < hi)
                    pack_chunk(acc, (const HPK_LDS_AS uint32_t*)sd, (const HPK_LDS_AS uint32_t*)ss, win_cnt, lo, hi, (lo + a.dst_mis) & 15u, a.src);
            }
            cur = rend > cur ? rend : cur;
        }
        if (have) pack_store(a.dst_base + c0 + 16u * tid, acc, (clo + a.dst_mis) & 15u, chi - clo);
    }
}
}  // namespace

size_t hpk_pack_tmp_bytes(uint32_t n) {
    const size_t nt = ((size_t)n + 1u + kLenTile - 1u) / kLenTile;
    return (nt + 1u) * 8u;
}

// dst_off = the exclusive sum of the n lengths (those passing src_cap counted 0), then the bytes end to
// end into dst_blob's first min(dst_off[n], dst_cap) bytes. tmp: hpk_pack_tmp_bytes(n) of device scratch.
// total_bound: no more than this many bytes can come out (it only sizes the grid).
int hpk_pack_launch(hpk_ctx* c, const uint8_t* src_blob, uint32_t src_cap, const uint32_t* src_off, const uint32_t* src_len,
                    uint32_t n, uint8_t* dst_blob, uint32_t dst_cap, uint32_t* dst_off, void* tmp, uint64_t total_bound) {
    const uint32_t nt = (uint32_t)(((uint64_t)n + 1u + kLenTile - 1u) / kLenTile);
    uint64_t* sums = static_cast<uint64_t*>(tmp);
    hipLaunchKernelGGL(pack_len_sums, dim3(nt), dim3(kLenT), 0, c->stream, src_off, src_len, n, src_cap, sums);
    hipLaunchKernelGGL(pack_sums_scan, dim3(1), dim3(kLenT), 0, c->stream, sums, nt);
    hipLaunchKernelGGL(pack_len_scan, dim3(nt), dim3(kLenT), 0, c->stream, src_off, src_len, n, src_cap,
                       (const uint64_t*)sums, nt, dst_off, c->d_err);
    HIP_TRY(hipGetLastError());
    uint64_t bytes = total_bound < dst_cap ? total_bound : dst_cap;
    if (bytes == 0 || n == 0) return HPK_E_OK;
    PackArgs a;
    const uintptr_t sp = (uintptr_t)src_blob, dp = (uintptr_t)dst_blob;
    a.src.base = (const uint32_t*)(sp & ~(uintptr_t)15);
    a.src.mis = (uint32_t)(sp & 15);
    a.src.cap = src_cap;
    a.src_off = src_off;
    a.dst_off = dst_off;
    a.n = n;
    a.dst_base = (uint8_t*)(dp & ~(uintptr_t)15);
    a.dst_mis = (uint32_t)(dp & 15);
    a.dst_cap = dst_cap;
    // a workgroup takes a contiguous run of tiles: 8 workgroups per CU when there are tiles enough
    const uint64_t tiles = (bytes + 15u + kPackTile - 1u) / kPackTile;
    uint64_t grid = (tiles + 3u) / 4u;
    const uint64_t most = (uint64_t)c->num_cu * 8u;
    grid = grid > most ? most : grid;
    hipLaunchKernelGGL(hpk_pack, dim3((uint32_t)grid), dim3(kPackThreads), kPackLdsBytes, c->stream, a);
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}

extern "C" int hpk_test_pack_geometry(uint32_t* tile_bytes, uint32_t* lds_literals) {
    if (!tile_bytes || !lds_literals) return HPK_E_INVAL;
    *tile_bytes = kPackTile;
    *lds_literals = kPackLds;
    return HPK_E_OK;
}
