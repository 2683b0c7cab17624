// hpk_pack.hip — the ordered pack: literals held anywhere in a source blob laid end to end, in literal
// order, with no gap (hpk_decode_batch_packed's last step, and hpk_pack_batch on its own). The result is
// what the reference's exact-length Vecs (huffman.rs:98, 160) would be, concatenated.
//
// Two steps on the context's stream:
//   * the length scan: dst_off = the exclusive u32 sum of the n lengths (n + 1 entries), the tiled scan
//     of hpk_scan.h over LenElem. A literal that passes the source capacity counts 0 bytes (and sets the
//     sticky error flag); the tile sums are 64-bit, and a total past HPK_MAX_OFFSET makes every offset 0
//     (flag set), so dst_off is always non-decreasing and the pack below never meets a wrapped offset;
//   * hpk_pack (per-thread code in hpk_pack.h): destination-centric. The destination, counted from its
//     16-byte-aligned base, is cut into tiles of kPackTile bytes; a workgroup takes a contiguous run of
//     tiles, finds its first literal by one binary search of dst_off, and from then on keeps a window
//     of up to kPackLds literals' dst_off / src_off in LDS, restaged when the tiles have used it up
//     (so each offset is read once per workgroup, and a tile that covers more literals than the window
//     holds is made in rounds). Each thread makes one aligned 16-byte chunk per tile and stores it
//     whole; the partial chunks at a misaligned start, at dst_off[n] and at the capacity go bytewise.
//     Bytes at or past min(dst_off[n], dst_cap) are never written.
//
// The bound scan lives here too (hpk_bound_scan, the same tiled scan over BoundElem): the region layout
// the packed form decodes into before it packs, and the workgroup-fill kernel's compacted layout.
#include "hpk_device.h"
#include "hpk_pack.h"
#include "hpk_scan.h"

using namespace hpkpack;

namespace {
using hpkscan::kK;
using hpkscan::kT;
using hpkscan::kTile;

// The bound layout's element: the 4-rounded decoded bound of literal i from two neighbouring offsets,
// clamped to 2^31 - 1; its sums are mod 2^32. The tile's offsets are staged in LDS (striped, coalesced), so
// that each is read once: element l's bound = s[l + 1] - s[l] rounded.
struct BoundElem {
    const uint32_t* __restrict__ off;

    static __device__ __forceinline__ uint32_t bound_of(uint32_t a, uint32_t b) {
        const uint64_t nb = (uint64_t)(b - a);  // (decreasing offsets: the decode kernel reports them)
        const uint64_t bd = ((nb * 8u) / 5u + 3u) & ~(uint64_t)3u;
        return bd > 0x7FFFFFFFu ? 0x7FFFFFFFu : (uint32_t)bd;
    }
    __device__ __forceinline__ void tile(uint32_t n, uint32_t base, uint32_t* s, uint32_t (&v)[kK]) const {
        const uint32_t t = threadIdx.x;
#pragma unroll
        for (uint32_t k = 0; k < kK; ++k) {
            const uint32_t j = base + t + kT * k;
            s[t + kT * k] = j <= n ? off[j] : 0u;
        }
        if (t == 0) s[kTile] = base + kTile <= n ? off[base + kTile] : 0u;
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < kK; ++k) {
            const uint32_t l = t * kK + k;
            v[k] = base + l < n ? bound_of(s[l], s[l + 1]) : 0u;
        }
    }
    __device__ __forceinline__ uint32_t tile_sum(uint32_t n, uint32_t base, uint32_t* s) const {
        uint32_t v[kK], acc = 0;
        tile(n, base, s, v);
#pragma unroll
        for (uint32_t k = 0; k < kK; ++k) acc += v[k];
        return acc;
    }
};

// The pack's element: piece i's length, 0 when its bytes would pass the source capacity (the sticky error
// flag is then set, by the tile scan). A thread loads all its offsets and lengths before it uses any.
struct LenElem {
    const uint32_t* __restrict__ off;
    const uint32_t* __restrict__ len;
    uint32_t cap;
    uint32_t* err;

    // the thread's striped elements base + threadIdx.x + kT * k into w; true: one of them passes the capacity
    __device__ __forceinline__ bool load(uint32_t n, uint32_t base, uint32_t (&w)[kK]) const {
        uint32_t o[kK], l[kK];
#pragma unroll
        for (uint32_t k = 0; k < kK; ++k) {
            const uint32_t j = base + threadIdx.x + kT * k;
            o[k] = j < n ? off[j] : 0u;
            l[k] = j < n ? len[j] : 0u;
        }
        bool bad = false;
#pragma unroll
        for (uint32_t k = 0; k < kK; ++k) {
            const bool ok = l[k] == 0u || (o[k] <= cap && l[k] <= cap - o[k]);
            bad |= !ok;
            w[k] = ok ? l[k] : 0u;
        }
        return bad;
    }
    __device__ __forceinline__ void tile(uint32_t n, uint32_t base, uint32_t* s, uint32_t (&v)[kK]) const {
        const uint32_t t = threadIdx.x;
        uint32_t w[kK];
        if (load(n, base, w)) *err = 1u;
#pragma unroll
        for (uint32_t k = 0; k < kK; ++k) s[t + kT * k] = w[k];
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < kK; ++k) v[k] = s[t * kK + k];
    }
    __device__ __forceinline__ uint64_t tile_sum(uint32_t n, uint32_t base, uint32_t*) const {
        uint32_t w[kK];
        (void)load(n, base, w);
        uint64_t acc = 0;
#pragma unroll
        for (uint32_t k = 0; k < kK; ++k) acc += w[k];
        return acc;
    }
};

// The packed encode's element: literal i's encoded length as the length pass wrote it (checked there).
struct EncLenElem {
    const uint32_t* __restrict__ len;

    __device__ __forceinline__ void tile(uint32_t n, uint32_t base, uint32_t* s, uint32_t (&v)[kK]) const {
        const uint32_t t = threadIdx.x;
#pragma unroll
        for (uint32_t k = 0; k < kK; ++k) {
            const uint32_t j = base + t + kT * k;
            s[t + kT * k] = j < n ? len[j] : 0u;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < kK; ++k) v[k] = s[t * kK + k];
    }
    __device__ __forceinline__ uint64_t tile_sum(uint32_t n, uint32_t base, uint32_t*) const {
        uint64_t acc = 0;
#pragma unroll
        for (uint32_t k = 0; k < kK; ++k) {
            const uint32_t j = base + threadIdx.x + kT * k;
            acc += j < n ? len[j] : 0u;
        }
        return acc;
    }
};

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

// (hpk_pack2 in hpk_decode_strings.hip is this kernel's twin, with a source selector staged beside each window's
// offsets: a fix to the tile loop or the window restaging below belongs in both)

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

size_t hpk_bound_tmp_bytes(uint32_t n) { return hpkscan::tmp_bytes<uint32_t>(n); }

int hpk_bound_scan(hpk_ctx* c, const uint32_t* in_off, uint32_t n, uint32_t* out, void* tmp) {
    hpkscan::launch<uint32_t>(c->stream, BoundElem{in_off}, n, out, tmp, nullptr);
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}

// (tests only) the bound layout of device offsets into device memory, synchronously
extern "C" int hpk_test_bound_scan(hpk_ctx* c, const uint32_t* in_off, uint32_t n, uint32_t* out) {
    void* t = nullptr;
    HIP_TRY(hipMalloc(&t, hpk_bound_tmp_bytes(n)));
    const int rc = hpk_bound_scan(c, in_off, n, out, t);
    const hipError_t e = hipStreamSynchronize(c->stream);
    (void)hipFree(t);
    return rc ? rc : e == hipSuccess ? HPK_E_OK : HPK_E_DEVICE;
}

size_t hpk_pack_tmp_bytes(uint32_t n) { return hpkscan::tmp_bytes<uint64_t>(n); }

int hpk_len_scan(hpk_ctx* c, const uint32_t* len, uint32_t n, uint32_t* out_off, void* tmp) {
    hpkscan::launch<uint64_t>(c->stream, EncLenElem{len}, n, out_off, tmp, c->d_err);
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}

const unsigned long long* hpk_len_scan_verdict(const void* tmp, uint32_t n) {
    return static_cast<const unsigned long long*>(tmp) + hpkscan::tiles(n);  // (sums[nt], hpk_scan.h)
}

// dst_off = the exclusive sum of the n lengths (those passing src_cap counted 0), then the bytes end to
// end into dst_blob's first min(dst_off[n], dst_cap) bytes. tmp: hpk_pack_tmp_bytes(n) of device scratch.
// total_bound: no more than this many bytes can come out (it only sizes the grid).
int hpk_pack_launch(hpk_ctx* c, const uint8_t* src_blob, uint32_t src_cap, const uint32_t* src_off, const uint32_t* src_len,
                    uint32_t n, uint8_t* dst_blob, uint32_t dst_cap, uint32_t* dst_off, void* tmp, uint64_t total_bound) {
    hpkscan::launch<uint64_t>(c->stream, LenElem{src_off, src_len, src_cap, c->d_err}, n, dst_off, tmp, c->d_err);
    HIP_TRY(hipGetLastError());
    uint64_t bytes = total_bound < dst_cap ? total_bound : dst_cap;
    if (bytes == 0 || n == 0) return HPK_E_OK;
    const auto src = split16(src_blob);
    const auto dst = split16(dst_blob);
    PackArgs a;
    a.src.base = (const uint32_t*)src.base;
    a.src.mis = src.mis;
    a.src.cap = src_cap;
    a.src_off = src_off;
    a.dst_off = dst_off;
    a.n = n;
    a.dst_base = dst.base;
    a.dst_mis = dst.mis;
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
