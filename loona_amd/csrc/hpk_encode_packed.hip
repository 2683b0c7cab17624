// hpk_encode_packed.hip — the packed encode's kernels (hpk_encode_batch_packed, hpk_encoded_len_batch): the length
// pass (hpk_enclen, below) and the packed instantiation of the encode tile kernel (hpk_encode2 with kPacked,
// hpk_encode_kernel.h). The length scan between them is in hpk_pack.hip. A translation unit of its own: the
// region form's kernel stays alone in hpk_encode.hip's module.
#include "hpk_encode_kernel.h"

namespace {

// ---------------------------------------------------------------------------------------------
// The length pass (hpk_encoded_len_batch, and the packed form's first step): out_len[i] = the encoded
// bytes of literal i, ceil(code bits / 8), with no byte encoded. hpk_encode2 without its image: a workgroup
// takes a byte-balanced literal range (split_by_bytes) and walks it in tiles of kEB * 32 input bytes, each
// thread holding 32 bytes of the tile (two 16-byte loads). No output has to fit anything, so a tile is a
// stretch of input, not a set of whole literals:
//   * every thread writes the running sums of its 32 bytes' code lengths to LDS (rel, u16), and a scan of
//     the threads' totals over the workgroup (the DPP scan of hpk_encode2) gives each thread's base (pre):
//     P(x) = pre[x / 32] + rel[x] is the code bits of the tile's bytes before byte x;
//   * one thread per literal then takes the difference of P at the literal's two ends (offsets checked as
//     they are read, up to kEQ literals a tile);
//   * a literal that passes the tile's end carries its bits so far into the next tile (64-bit), which
//     starts where this one ended: a literal of any size is summed by the whole workgroup.
// A literal with bad offsets gets length 0 (status HPK_BAD_OFFSETS where a status array is given) and sets
// the sticky flag; it voids no other literal. The tile that meets one hands its window of up to kEQ literals
// to a loop of one literal per lane (rare path: the literals around a bad one may overlap in the input,
// which no tile can hold), and the tiled walk starts again at the literal after the window.
struct EncLenArgs {
    const uint8_t* in_blob;
    const uint8_t* in_base;  // 16-byte aligned
    uint32_t in_mis, in_cap;
    const uint32_t* in_off;
    uint32_t n;
    uint32_t* out_len;
    uint8_t* status;  // may be null
    const uint32_t* codes;
    uint32_t* err;
};

template <int kEB, int kEQ>
struct EncLenLds {
    uint16_t rel[kEB * 32];  // code bits of the thread's bytes before this one
    uint32_t pre[kEB + 1];   // code bits of the tile's bytes before the thread's; [kEB]: the tile's total
    uint8_t len1[256];
    uint32_t wsum[16];       // per-wave totals
    uint32_t ctr[4];         // [0] the window's first literal that passes the tile's end (the window's count
                             // if none), [1] bad offsets seen, [2], [3] that literal's bits so far
    uint32_t split[2 * hpksplit::kMaxRounds];
};

__device__ __forceinline__ uint32_t enclen_bytes(uint64_t bits) {
    const uint64_t nb = (bits + 7u) >> 3;
    return nb > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)nb;  // (such a batch's total passes HPK_MAX_OFFSET)
}

template <int kEB, int kEQ>
__global__ __launch_bounds__(kEB, 4) void hpk_enclen(EncLenArgs a) {
    constexpr uint32_t kTile = kEB * 32;
    constexpr int kEMeta = kEQ / kEB;
    static_assert(kEB % 64 == 0 && kEB <= 1024 && kEQ % kEB == 0, "geometry");
    __shared__ __attribute__((aligned(16))) EncLenLds<kEB, kEQ> S;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    if (tid < 256) S.len1[tid] = (uint8_t)a.codes[257 + tid];
    if (tid < 4) S.ctr[tid] = 0;
    uint32_t BA, BB;
    hpksplit::split_by_bytes<kEB, 16>(a.in_off, a.n, S.split, BA, BB);  // (barriers: the table is in place)
    const uint32_t in_end = a.in_cap + a.in_mis;  // loads are clamped to the blob's last 16-byte chunk
    const uint32_t last16 = in_end ? (in_end - 1) >> 4 : 0;
    const uint4* g_in = reinterpret_cast<const uint4*>(a.in_base);
    uint32_t cur = BA;   // the first literal not yet summed
    uint32_t pos = 0;    // where the tile's bytes start (base-relative: + mis): literal cur's start, or the
    uint64_t acc = 0;    // previous tile's end with acc = literal cur's bits before it
    if (cur < BB) pos = a.in_off[cur] + a.in_mis;
    while (cur < BB) {  // block-uniform
        const uint32_t cnt = min((uint32_t)kEQ, BB - cur);
        const uint32_t base16 = pos & ~15u;
        const uint32_t c0 = (base16 >> 4) + 2u * tid;
        const uint4 ch0 = g_in[min(c0, last16)], ch1 = g_in[min(c0 + 1u, last16)];
        uint32_t pi0[kEMeta], pi1[kEMeta];
        bool bad = false;
#pragma unroll
        for (int r = 0; r < kEMeta; ++r) {
            const uint32_t t = min(tid + (uint32_t)kEB * r, cnt - 1u);
            pi0[r] = a.in_off[cur + t];
            pi1[r] = a.in_off[cur + t + 1];
        }
#pragma unroll
        for (int r = 0; r < kEMeta; ++r)
            bad |= tid + (uint32_t)kEB * r < cnt && !(pi0[r] <= pi1[r] && pi1[r] <= a.in_cap);
        if (__any(bad) && lane == 0) S.ctr[1] = 1u;
        // the thread's 32 code lengths: running sums to rel (pairs of u16, four 16-byte stores)
        const uint32_t wd[8] = {ch0.x, ch0.y, ch0.z, ch0.w, ch1.x, ch1.y, ch1.z, ch1.w};
        uint32_t v = 0;
        uint4* rel16 = reinterpret_cast<uint4*>(S.rel) + 4u * tid;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            uint32_t pk[4];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t ln = S.len1[(wd[2 * g + (j >> 2)] >> (8 * (j & 3))) & 0xFFu];
                pk[j >> 1] = (j & 1) ? pk[j >> 1] | (v << 16) : v;  // (v <= 31 * 30)
                v += ln;
            }
            rel16[g] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        }
        uint32_t f = 0, vi = v, L = 0;
        wave_seg_scan(f, vi, L, lane);  // (no segment starts: a plain inclusive sum)
        if (lane == 63) S.wsum[wv] = vi;
        lds_barrier_e();
        if (S.ctr[1]) {  // bad offsets in the window (block-uniform): its literals one per lane, then the tiled
            // walk starts again at the literal after the window
            bool flagged = false;
            for (uint32_t i = cur + tid; i < cur + cnt; i += kEB) {
                const uint32_t s = a.in_off[i], e = a.in_off[i + 1];
                const bool ok = s <= e && e <= a.in_cap;
                uint64_t bits = 0;
                if (ok)
                    for (uint32_t p = s; p < e; ++p) bits += S.len1[a.in_blob[p]];
                a.out_len[i] = enclen_bytes(bits);
                if (a.status) a.status[i] = (uint8_t)(ok ? HPK_OK : HPK_BAD_OFFSETS);
                flagged |= !ok;
            }
            if (__any(flagged) && lane == 0) *a.err = 1u;
            lds_barrier_e();  // every thread has read the flag
            if (tid == 0) S.ctr[1] = 0;
            cur += cnt;
            acc = 0;
            if (cur < BB) pos = a.in_off[cur] + a.in_mis;
            lds_barrier_e();  // (cleared before the next window's check can set it)
            continue;
        }
        uint32_t cw = 0;
#pragma unroll
        for (uint32_t j = 0; j < (uint32_t)kEB / 64u - 1u; ++j) {
            const uint32_t s = S.wsum[j];
            if (j < wv) cw += s;
        }
        S.pre[tid] = cw + vi - v;
        if (tid == (uint32_t)kEB - 1u) S.pre[kEB] = cw + vi;
        if (tid == 0) S.ctr[0] = cnt;  // (every thread has read the previous tile's: it passed the barrier above)
        lds_barrier_e();
        auto P = [&](uint32_t x) { return x < kTile ? S.pre[x >> 5] + (uint32_t)S.rel[x] : S.pre[kEB]; };
#pragma unroll
        for (int r = 0; r < kEMeta; ++r) {
            const uint32_t t = tid + (uint32_t)kEB * r;
            if (t < cnt) {
                const uint32_t i0 = pi0[r] + a.in_mis, i1 = pi1[r] + a.in_mis;
                // (literal 0 may have started in an earlier tile: i0 < pos; the others start at or after pos)
                const uint32_t xs = (t == 0 ? pos : i0) - base16;
                const bool starts = t == 0 || xs <= kTile;  // the literal before this one ends in the tile
                const bool ends = starts && i1 - base16 <= kTile;
                const uint64_t before = t == 0 ? acc : 0ull;
                if (ends) {
                    a.out_len[cur + t] = enclen_bytes(before + (uint64_t)(P(i1 - base16) - P(xs)));
                    if (a.status) a.status[cur + t] = (uint8_t)HPK_OK;
                } else if (starts) {  // the one literal that passes the tile's end
                    const uint64_t part = before + (uint64_t)(S.pre[kEB] - P(xs));
                    S.ctr[0] = t;
                    S.ctr[2] = (uint32_t)part;
                    S.ctr[3] = (uint32_t)(part >> 32);
                }
            }
        }
        lds_barrier_e();
        const uint32_t k = S.ctr[0];
        cur += k;
        if (k == cnt) {  // every literal of the window ended: the next tile starts at the next literal
            acc = 0;
            if (cur < BB) pos = a.in_off[cur] + a.in_mis;
        } else {
            acc = ((uint64_t)S.ctr[3] << 32) | S.ctr[2];
            pos = base16 + kTile;
        }
    }
}

}  // namespace

// The encode proper into b.out_off's exact regions; void_all: the length scan's verdict on the total.
int hpk_launch_encode_packed(hpk_ctx* c, const hpk_batch& b, const unsigned long long* void_all) {
    EncodeArgs a{b.in_blob, b.in_off, b.n, b.out_blob, b.out_off, b.out_len, b.status, c->d_codes};
    const auto in = split16(b.in_blob);
    const auto out = split16(b.out_blob);
    a.in_base = in.base;
    a.in_mis = in.mis;
    a.out_base = out.base;
    a.out_mis = out.mis;
    a.in_cap = b.in_cap;
    a.out_cap = b.out_cap;
    a.err = c->d_err;
    a.prof = nullptr;
    a.void_all = void_all;
    // the region form's grid (hpk_launch_encode): two workgroups per CU, at least kProdPerWg literals each
    uint64_t blocks = ((uint64_t)b.n + kProdPerWg - 1u) / kProdPerWg;
    const uint64_t cus = (uint64_t)c->num_cu - (c->sm_launched && c->sm_max ? (uint64_t)c->sm_wgs : 0u);
    if (blocks > cus * 2u) blocks = cus * 2u;
    if (blocks < 1) blocks = 1;
    const dim3 grid((uint32_t)blocks);
#ifdef HPK_DIAG
    const char* w = getenv("HPK_ENCODE_CFG");
    if (w && atoi(w) == 9) {  // the packed instantiation with per-phase cycle counters (hpk_debug_encode_prof)
        if (!hpk_g_eprof) HIP_TRY(hipMalloc(&hpk_g_eprof, 16 * sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(hpk_g_eprof, 0, 16 * sizeof(unsigned long long), c->stream));
        a.prof = hpk_g_eprof;
        hipLaunchKernelGGL((hpk_encode2<kProdEB, kProdEO, kProdEQ, kProdEBytes, 1, 1>), grid, dim3(kProdEB), 0, c->stream,
                           a);
        HIP_TRY(hipGetLastError());
        return HPK_E_OK;
    }
#endif
    hipLaunchKernelGGL((hpk_encode2<kProdEB, kProdEO, kProdEQ, kProdEBytes, 0, 1>), grid, dim3(kProdEB), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}

int hpk_launch_enclen(hpk_ctx* c, const uint8_t* in_blob, uint32_t in_cap, const uint32_t* in_off, uint32_t n,
                      uint32_t* out_len, uint8_t* status) {
    const auto in = split16(in_blob);
    const EncLenArgs a{in_blob, in.base, in.mis, in_cap, in_off, n, out_len, status, c->d_codes, c->d_err};
    // four workgroups per CU (35 KiB of LDS and 38 VGPRs each: they fit), at least kProdPerWg literals each
    uint64_t blocks = ((uint64_t)n + kProdPerWg - 1u) / kProdPerWg;
    const uint64_t cus = (uint64_t)c->num_cu - (c->sm_launched && c->sm_max ? (uint64_t)c->sm_wgs : 0u);
    if (blocks > cus * 4u) blocks = cus * 4u;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL((hpk_enclen<kProdEB, kProdEQ>), dim3((uint32_t)blocks), dim3(kProdEB), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}

extern "C" int hpk_test_enclen_geometry(uint32_t* stretch_bytes, uint32_t* window_literals, uint32_t* one_wg_literals) {
    if (!stretch_bytes || !window_literals || !one_wg_literals) return HPK_E_INVAL;
    *stretch_bytes = kProdEB * 32;
    *window_literals = kProdEQ;
    *one_wg_literals = kProdPerWg;
    return HPK_E_OK;
}
