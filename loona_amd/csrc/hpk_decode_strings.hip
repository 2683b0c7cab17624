// hpk_decode_strings.hip — the packed string-literal decode's own kernels (hpk_decode_strings_packed): RFC 7541
// §5.2 string literals as decode_string reads them (crates/loona-hpack/src/decoder.rs:135-163), each in a window
// of the input blob, raw and Huffman mixed, coming back end to end. A translation unit of its own: the decode
// kernels and the ordered pack stay alone in their modules. The call's steps (hpk_calls_strings.hip strings them together):
//   * hpk_strparse below, one thread per string (per-thread code in hpk_strparse.h): the length integer, the
//     length check and the H bit give a parse status, the payload's start, `consumed`, and two lengths of which
//     at most one is nonzero: hlen (a Huffman payload's bytes) and rlen (a raw payload's);
//   * hpk_pack_launch (hpk_pack.hip, as it is) gathers the Huffman payloads (in_blob, start, hlen) into a
//     contiguous blob with offsets hoff: raw and void strings are empty literals there;
//   * hpk_bound_scan and hpk_launch_decode (as they are): the region decode of that blob into scratch;
//   * hpk_strmerge below, elementwise: the final out_len and status, and per string the source of its bytes
//     (the region scratch at its bound offset, or the input blob at its payload's start);
//   * hpk_len_scan (as it is) writes out_off;
//   * hpk_pack2 below: hpk_pack's tile loop with a source per literal (pack2_chunk, hpk_pack.h), the selector
//     staged in LDS beside each window of offsets.
#include "hpk_device.h"
#include "hpk_pack.h"
#include "hpk_strparse.h"

using namespace hpkpack;

namespace {

struct StrParseArgs {
    const uint8_t* in_blob;
    uint32_t in_cap;
    const uint32_t* str_off;
    const uint32_t* str_end;
    uint32_t n;
    uint32_t* start;
    uint32_t* hlen;
    uint32_t* rlen;
    uint8_t* pst;
    uint32_t* consumed;  // may be null
    uint32_t* err;
};

__global__ __launch_bounds__(256) void hpk_strparse(StrParseArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const hpkstr::StrParse r = hpkstr::str_parse(a.in_blob, a.in_cap, a.str_off[i], a.str_end[i]);
    if (r.status == HPK_BAD_OFFSETS) *a.err = 1u;
    a.start[i] = r.start;
    a.hlen[i] = r.huff ? r.len : 0u;
    a.rlen[i] = r.huff ? 0u : r.len;
    a.pst[i] = (uint8_t)r.status;
    if (a.consumed) a.consumed[i] = r.consumed;
}

struct StrMergeArgs {
    uint32_t n;
    uint32_t* src;  // in: the payload's start; out: the source offset of the string's bytes
    const uint32_t* hlen;
    const uint32_t* rlen;
    const uint8_t* pst;
    const uint32_t* hoff;   // the gathered Huffman blob's offsets, n + 1
    const uint32_t* bound;  // the region layout, n + 1
    uint32_t region_cap;
    uint32_t* out_len;  // in: the region decode's; out: the final ones
    uint8_t* status;
    uint8_t* sel;  // out: 0 the region scratch, 1 the input blob
    uint32_t* err;
};

__global__ __launch_bounds__(256) void hpk_strmerge(StrMergeArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t ps = a.pst[i], hl = a.hlen[i];
    uint32_t len = 0, st = ps, src = 0, sel = 0;
    if (ps == HPK_OK && hl != 0u) {  // a Huffman payload: the decode's result, where the gather held all of it
        const uint32_t b = a.bound[i];
        len = a.out_len[i];
        st = a.status[i];
        src = b;
        const bool whole = a.hoff[i + 1] - a.hoff[i] == hl;  // (not when the payloads' total passed the gather's capacity)
        if (!whole || b > a.region_cap || len > a.region_cap - b) {
            len = 0;
            st = HPK_BAD_OFFSETS;
            src = 0;
            *a.err = 1u;
        }
    } else if (ps == HPK_OK) {  // raw (or an empty Huffman payload): the payload as it is
        len = a.rlen[i];
        src = a.src[i];
        sel = 1;
    }
    a.out_len[i] = len;
    a.status[i] = (uint8_t)st;
    a.src[i] = src;
    a.sel[i] = (uint8_t)sel;
}

struct Pack2Args {
    PackSrc src0, src1;
    const uint32_t* src_off;
    const uint8_t* sel;
    const uint32_t* dst_off;
    uint32_t n;
    uint8_t* dst_base;  // 16-byte aligned: the blob starts dst_mis bytes in
    uint32_t dst_mis;
    uint32_t dst_cap;
};

constexpr uint32_t kPack2LdsBytes = (2u * kPackLds + 4u) * 4u + kPackLds;

// hpk_pack (hpk_pack.hip) with the window's selectors staged beside its offsets: the same tile loop line for line
// but for vx / sx and pack2_chunk, kept apart so that hpk_pack's code stays as it is; a fix to one belongs in both
__global__ __launch_bounds__(kPackThreads) void hpk_pack2(Pack2Args a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t pack2_smem[];
    uint32_t* sd = pack2_smem;                 // the window's dst_off, kPackLds + 1 entries
    uint32_t* ss = pack2_smem + kPackLds + 4;  // its src_off
    uint8_t* sx = reinterpret_cast<uint8_t*>(pack2_smem + 2u * kPackLds + 4u);  // its selectors
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
    uint32_t win_a = pack_upper(a.dst_off, n + 1u, (uint32_t)((c_first > a.dst_mis ? c_first : a.dst_mis) - a.dst_mis)) - 1u;
    uint32_t win_cnt = 0;
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
                uint32_t vd[kPackLds / kPackThreads], vs[kPackLds / kPackThreads], vx[kPackLds / kPackThreads];
#pragma unroll
                for (uint32_t i = 0; i < kPackLds / kPackThreads; ++i) {  // (all the loads first)
                    const uint32_t j = tid + kPackThreads * i;
                    vd[i] = j < win_cnt ? a.dst_off[win_a + j] : 0u;
                    vs[i] = j < win_cnt ? a.src_off[win_a + j] : 0u;
                    vx[i] = j < win_cnt ? a.sel[win_a + j] : 0u;
                }
                if (tid == 0) sd[win_cnt] = a.dst_off[win_a + win_cnt];
#pragma unroll
                for (uint32_t i = 0; i < kPackLds / kPackThreads; ++i) {
                    const uint32_t j = tid + kPackThreads * i;
                    if (j < win_cnt) {
                        sd[j] = vd[i];
                        ss[j] = vs[i];
                        sx[j] = (uint8_t)vx[i];
                    }
                }
                __syncthreads();
            }
            const uint32_t we = sd[win_cnt];
            const uint32_t rend = we < thi ? we : thi;  // this round: offsets [cur, rend)
            if (have) {
                const uint32_t lo = clo > cur ? clo : cur, hi = chi < rend ? chi : rend;
                if (lo < hi)
                    pack2_chunk(acc, (const HPK_LDS_AS uint32_t*)sd, (const HPK_LDS_AS uint32_t*)ss, (const HPK_LDS_AS uint8_t*)sx,
                                win_cnt, lo, hi, (lo + a.dst_mis) & 15u, a.src0, a.src1);
            }
            cur = rend > cur ? rend : cur;
        }
        if (have) pack_store(a.dst_base + c0 + 16u * tid, acc, (clo + a.dst_mis) & 15u, chi - clo);
    }
}
}  // namespace

int hpk_launch_strparse(hpk_ctx* c, const uint8_t* in_blob, uint32_t in_cap, const uint32_t* str_off, const uint32_t* str_end,
                        uint32_t n, uint32_t* start, uint32_t* hlen, uint32_t* rlen, uint8_t* pst, uint32_t* consumed) {
    const StrParseArgs a{in_blob, in_cap, str_off, str_end, n, start, hlen, rlen, pst, consumed, c->d_err};
    hipLaunchKernelGGL(hpk_strparse, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}

int hpk_launch_strmerge(hpk_ctx* c, uint32_t n, uint32_t* src, const uint32_t* hlen, const uint32_t* rlen, const uint8_t* pst,
                        const uint32_t* hoff, const uint32_t* bound, uint32_t region_cap, uint32_t* out_len, uint8_t* status,
                        uint8_t* sel) {
    const StrMergeArgs a{n, src, hlen, rlen, pst, hoff, bound, region_cap, out_len, status, sel, c->d_err};
    hipLaunchKernelGGL(hpk_strmerge, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}

int hpk_pack2_launch(hpk_ctx* c, const uint8_t* src0, uint32_t cap0, const uint8_t* src1, uint32_t cap1, const uint32_t* src_off,
                     const uint8_t* sel, uint32_t n, uint8_t* dst_blob, uint32_t dst_cap, const uint32_t* dst_off,
                     uint64_t total_bound) {
    const uint64_t bytes = total_bound < dst_cap ? total_bound : dst_cap;
    if (bytes == 0 || n == 0) return HPK_E_OK;
    const auto s0 = split16(src0), s1 = split16(src1);
    const auto dst = split16(dst_blob);
    Pack2Args a;
    a.src0 = PackSrc{(const uint32_t*)s0.base, s0.mis, cap0};
    a.src1 = PackSrc{(const uint32_t*)s1.base, s1.mis, cap1};
    a.src_off = src_off;
    a.sel = sel;
    a.dst_off = dst_off;
    a.n = n;
    a.dst_base = dst.base;
    a.dst_mis = dst.mis;
    a.dst_cap = dst_cap;
    // (the grid as hpk_pack_launch's; the kernel cuts the tiles of the true total over whatever grid it gets)
    const uint64_t tiles = (bytes + 15u + kPackTile - 1u) / kPackTile;
    uint64_t grid = (tiles + 3u) / 4u;
    const uint64_t most = (uint64_t)c->num_cu * 8u;
    grid = grid > most ? most : grid;
    hipLaunchKernelGGL(hpk_pack2, dim3((uint32_t)grid), dim3(kPackThreads), kPack2LdsBytes, c->stream, a);
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}
