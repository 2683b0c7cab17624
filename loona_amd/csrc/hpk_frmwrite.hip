// hpk_frmwrite.hip — the frame write (hpk_write_frames): header blocks held end to end in a source blob become
// what goes on the wire, one HEADERS frame and the CONTINUATION frames the peer's SETTINGS_MAX_FRAME_SIZE demands
// per block (the reference's loop in send_data_maybe, crates/loona/src/h2/server.rs:470-508, with
// Frame::write_into's header, crates/loona-h2/src/lib.rs:413-422), block after block with no gap.
//
// Three steps on the context's stream:
//   * the length scan: wire_off = the exclusive u32 sum of the blocks' wire lengths (n + 1 entries), the tiled scan
//     of hpk_scan.h over FwLenElem. A void block (offsets that decrease or pass the capacity, a frame size of 0 or
//     above 0xFFFFFF) counts 0 octets and sets the sticky flag; the tile sums are 64-bit, and a total past
//     HPK_MAX_OFFSET makes every offset 0 (flag set);
//   * hpk_frmstatus, elementwise: status[b] = HPK_BAD_OFFSETS for a void block, and for every block when the scan's
//     verdict word says that the total did not fit, else HPK_OK;
//   * hpk_frmwrite (per-thread code in hpk_frmwrite.h): destination-centric, the ordered pack's tile loop. The
//     destination, counted from its 16-byte-aligned base, is cut into tiles of kFwTile bytes; a workgroup takes a
//     contiguous run of tiles, finds its first block by one binary search of wire_off, and keeps a window of up to
//     kFwLds blocks' wire_off / block_off / max_frame / stream_id in LDS, restaged when the tiles have used it up.
//     Each thread makes one aligned 16-byte chunk per tile and stores it whole; the partial chunks at a misaligned
//     start, at wire_off[n] and at the capacity go bytewise. Octets at or past min(wire_off[n], out_cap) are never
//     written.
#include "hpk_device.h"
#include "hpk_frmwrite.h"
#include "hpk_scan.h"

using namespace hpkfw;
using hpkpack::pack_chunk_range;
using hpkpack::pack_store;
using hpkpack::pack_upper;

namespace {
using hpkscan::kK;
using hpkscan::kT;
using hpkscan::kTile;

// The scan's element: block i's wire length from block_off[i], block_off[i + 1] and max_frame[i], 0 for a void
// block (the tile scan then sets the sticky flag). A thread loads all its offsets and frame sizes before it uses
// any. The tile scan's values are the lengths mod 2^32: it uses them only when the 64-bit total fits.
struct FwLenElem {
    const uint32_t* __restrict__ off;
    const uint32_t* __restrict__ mf;
    uint32_t cap;
    uint32_t* err;

    // the thread's striped elements base + threadIdx.x + kT * k into w; true: one of them is void
    __device__ __forceinline__ bool load(uint32_t n, uint32_t base, uint64_t (&w)[kK]) const {
        uint32_t a[kK], e[kK], m[kK];
#pragma unroll
        for (uint32_t k = 0; k < kK; ++k) {
            const uint32_t j = base + threadIdx.x + kT * k;
            a[k] = j < n ? off[j] : 0u;
            e[k] = j < n ? off[j + 1u] : 0u;
            m[k] = j < n ? mf[j] : 1u;
        }
        bool bad = false;
#pragma unroll
        for (uint32_t k = 0; k < kK; ++k) {
            bad |= !fw_block_ok(a[k], e[k], m[k], cap);
            w[k] = fw_elem(a[k], e[k], m[k], cap);
        }
        return bad;
    }
    __device__ __forceinline__ void tile(uint32_t n, uint32_t base, uint32_t* s, uint32_t (&v)[kK]) const {
        const uint32_t t = threadIdx.x;
        uint64_t w[kK];
        if (load(n, base, w)) *err = 1u;
#pragma unroll
        for (uint32_t k = 0; k < kK; ++k) s[t + kT * k] = (uint32_t)w[k];
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < kK; ++k) v[k] = s[t * kK + k];
    }
    __device__ __forceinline__ uint64_t tile_sum(uint32_t n, uint32_t base, uint32_t*) const {
        uint64_t w[kK];
        (void)load(n, base, w);
        uint64_t acc = 0;
#pragma unroll
        for (uint32_t k = 0; k < kK; ++k) acc += w[k];
        return acc;
    }
};

__global__ __launch_bounds__(kT) void hpk_frmstatus(const uint32_t* __restrict__ off, const uint32_t* __restrict__ mf, uint32_t cap,
                                                    uint32_t n, const unsigned long long* __restrict__ void_all,
                                                    uint8_t* __restrict__ status) {
    const uint32_t b = blockIdx.x * kT + threadIdx.x;
    if (b >= n) return;
    const bool ok = *void_all == 0ull && fw_block_ok(off[b], off[b + 1u], mf[b], cap);
    status[b] = ok ? (uint8_t)HPK_OK : (uint8_t)HPK_BAD_OFFSETS;
}

struct FwArgs {
    PackSrc src;
    const uint32_t* block_off;
    const uint32_t* max_frame;
    const uint32_t* stream_id;
    const uint32_t* wire_off;
    uint32_t n;
    uint8_t* dst_base;  // 16-byte aligned: the blob starts dst_mis bytes in
    uint32_t dst_mis;
    uint32_t dst_cap;
};

// the window's wire_off and block_off (kFwLds + 1 entries each, padded to + 4), max_frame and stream_id
constexpr uint32_t kFwLdsBytes = (4u * kFwLds + 8u) * 4u;

// (the tile loop and the window restaging are hpk_pack's, hpk_pack.hip, with four staged arrays for its two: a fix
// there belongs here too)
__global__ __launch_bounds__(kFwThreads) void hpk_frmwrite(FwArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t fw_smem[];
    uint32_t* sw = fw_smem;                      // the window's wire_off, kFwLds + 1 entries
    uint32_t* sb = fw_smem + kFwLds + 4;         // its block_off, kFwLds + 1 entries
    uint32_t* sm = fw_smem + 2u * kFwLds + 8;    // its max_frame
    uint32_t* si = fw_smem + 3u * kFwLds + 8;    // its stream_id
    const uint32_t tid = threadIdx.x, n = a.n;
    const uint32_t total = a.wire_off[n];
    const uint32_t limit = total < a.dst_cap ? total : a.dst_cap;
    if (limit == 0u) return;
    const uint64_t end = (uint64_t)a.dst_mis + limit;  // in coordinates from dst_base
    const uint64_t ntiles = (end + kFwTile - 1u) / kFwTile;
    const uint64_t per = (ntiles + gridDim.x - 1u) / gridDim.x;
    const uint64_t t_first = (uint64_t)blockIdx.x * per;
    const uint64_t t_last = t_first + per < ntiles ? t_first + per : ntiles;
    if (t_first >= t_last) return;
    const uint64_t c_first = t_first * kFwTile;
    // the block that holds the run's first octet: wire_off[0] = 0 <= it < wire_off[n]
    uint32_t win_a = pack_upper(a.wire_off, n + 1u, (uint32_t)((c_first > a.dst_mis ? c_first : a.dst_mis) - a.dst_mis)) - 1u;
    uint32_t win_cnt = 0;  // blocks [win_a, win_a + win_cnt) are staged; wire_off[win_a] <= cur throughout
    for (uint64_t t = t_first; t < t_last; ++t) {
        const uint64_t c0 = t * kFwTile, c1 = c0 + kFwTile;
        const uint32_t thi = (uint32_t)((c1 < end ? c1 : end) - a.dst_mis);
        uint32_t cur = (uint32_t)((c0 > a.dst_mis ? c0 : a.dst_mis) - a.dst_mis);
        uint32_t clo = 0, chi = 0;
        const bool have = pack_chunk_range(c0, tid, a.dst_mis, end, &clo, &chi);
        uint32_t acc[4] = {0u, 0u, 0u, 0u};
        while (cur < thi) {
            if (win_cnt == 0u || sw[win_cnt] <= cur) {  // (uniform) the window is used up: the next blocks
                win_a += win_cnt;
                __syncthreads();
                win_cnt = n - win_a < kFwLds ? n - win_a : kFwLds;
                uint32_t vw[kFwLds / kFwThreads], vb[kFwLds / kFwThreads], vm[kFwLds / kFwThreads], vi[kFwLds / kFwThreads];
#pragma unroll
                for (uint32_t i = 0; i < kFwLds / kFwThreads; ++i) {  // (all the loads first)
                    const uint32_t j = tid + kFwThreads * i;
                    vw[i] = j < win_cnt ? a.wire_off[win_a + j] : 0u;
                    vb[i] = j < win_cnt ? a.block_off[win_a + j] : 0u;
                    vm[i] = j < win_cnt ? a.max_frame[win_a + j] : 0u;
                    vi[i] = j < win_cnt ? a.stream_id[win_a + j] : 0u;
                }
                if (tid == 0) {
                    sw[win_cnt] = a.wire_off[win_a + win_cnt];
                    sb[win_cnt] = a.block_off[win_a + win_cnt];
                }
#pragma unroll
                for (uint32_t i = 0; i < kFwLds / kFwThreads; ++i) {
                    const uint32_t j = tid + kFwThreads * i;
                    if (j < win_cnt) {
                        sw[j] = vw[i];
                        sb[j] = vb[i];
                        sm[j] = vm[i];
                        si[j] = vi[i];
                    }
                }
                __syncthreads();
            }
            const uint32_t we = sw[win_cnt];
            const uint32_t rend = we < thi ? we : thi;  // this round: offsets [cur, rend)
            if (have) {
                const uint32_t lo = clo > cur ? clo : cur, hi = chi < rend ? chi : rend;
                if (lo < hi)
                    fw_chunk(acc, (const HPK_LDS_AS uint32_t*)sw, (const HPK_LDS_AS uint32_t*)sb, (const HPK_LDS_AS uint32_t*)sm,
                             (const HPK_LDS_AS uint32_t*)si, win_cnt, lo, hi, (lo + a.dst_mis) & 15u, a.src);
            }
            cur = rend > cur ? rend : cur;
        }
        if (have) pack_store(a.dst_base + c0 + 16u * tid, acc, (clo + a.dst_mis) & 15u, chi - clo);
    }
}
}  // namespace

// wire_off = the exclusive sum of the n blocks' wire lengths (void ones counted 0), status, then the frames end to
// end into out_blob's first min(wire_off[n], out_cap) octets. tmp: hpk_pack_tmp_bytes(n) of device scratch.
int hpk_frmwrite_launch(hpk_ctx* c, const uint8_t* blocks, uint32_t cap, const uint32_t* block_off, uint32_t n,
                        const uint32_t* stream_id, const uint32_t* max_frame, uint8_t* out_blob, uint32_t out_cap,
                        uint32_t* wire_off, uint8_t* status, void* tmp) {
    hpkscan::launch<uint64_t>(c->stream, FwLenElem{block_off, max_frame, cap, c->d_err}, n, wire_off, tmp, c->d_err);
    HIP_TRY(hipGetLastError());
    if (n == 0) return HPK_E_OK;
    hipLaunchKernelGGL(hpk_frmstatus, dim3((n + kT - 1u) / kT), dim3(kT), 0, c->stream, block_off, max_frame, cap, n,
                       hpk_len_scan_verdict(tmp, n), status);
    HIP_TRY(hipGetLastError());
    // An estimate that only sizes the grid (the kernel takes its tile count from wire_off[n]): every source octet once
    // and a header per frame, a frame per octet or per block. Blocks that overlap in the source can give more; the
    // workgroups then take longer runs of tiles.
    uint64_t bytes = 10ull * cap + 9ull * n;
    bytes = bytes < out_cap ? bytes : out_cap;
    if (bytes == 0) return HPK_E_OK;
    const auto src = split16(blocks);
    const auto dst = split16(out_blob);
    FwArgs a;
    a.src.base = (const uint32_t*)src.base;
    a.src.mis = src.mis;
    a.src.cap = cap;
    a.block_off = block_off;
    a.max_frame = max_frame;
    a.stream_id = stream_id;
    a.wire_off = wire_off;
    a.n = n;
    a.dst_base = dst.base;
    a.dst_mis = dst.mis;
    a.dst_cap = out_cap;
    // a workgroup takes a contiguous run of tiles: 8 workgroups per CU when there are tiles enough
    const uint64_t tiles = (bytes + 15u + kFwTile - 1u) / kFwTile;
    uint64_t grid = (tiles + 3u) / 4u;
    const uint64_t most = (uint64_t)c->num_cu * 8u;
    grid = grid > most ? most : grid;
    hipLaunchKernelGGL(hpk_frmwrite, dim3((uint32_t)grid), dim3(kFwThreads), kFwLdsBytes, c->stream, a);
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}

extern "C" int hpk_test_frmwrite_geometry(uint32_t* tile_bytes, uint32_t* lds_blocks) {
    if (!tile_bytes || !lds_blocks) return HPK_E_INVAL;
    *tile_bytes = kFwTile;
    *lds_blocks = kFwLds;
    return HPK_E_OK;
}
