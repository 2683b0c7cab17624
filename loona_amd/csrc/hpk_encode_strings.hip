// hpk_encode_strings.hip — the packed string-literal encode's kernels (hpk_encode_strings_packed,
// hpk_string_len_batch): RFC 7541 §5.2 string literals, each the §5.1 length prefix (H bit in its first
// octet) followed by the Huffman or the raw payload, end to end (encode_string_literal, encoder.rs:296-307,
// with put_string's "Huffman where strictly shorter"). A translation unit of its own: the region and the packed
// encode's kernels stay alone in their modules. The call's three steps:
//   * the length and form pass: hpk_enclen (hpk_encode_packed.hip, as it is) writes every literal's Huffman
//     byte count, then hpk_strlen_form below turns it, the input length and the policy into out_len (the whole
//     representation, prefix included) and status, one thread per literal;
//   * hpk_len_scan (hpk_pack.hip, as it is) writes out_off and its verdict word;
//   * hpk_encode_str below writes every representation at its final place, clipped at out_cap.
// Nothing is kept between the steps but out_len and out_off: plen(x) + x is strictly increasing, so the emit
// step finds the prefix length and the payload length again from a representation's length, and the form from
// the payload length, the input length and the policy (str_form).
#include "hpk_encode_kernel.h"

namespace {

// octets of the 7-bit-prefix integer p (encode_integer_into, encoder.rs:93-122)
__device__ __forceinline__ uint32_t str_plen(uint32_t p) {
    return p < 127u ? 1u : p - 127u < (1u << 7) ? 2u : p - 127u < (1u << 14) ? 3u : p - 127u < (1u << 21) ? 4u
           : p - 127u < (1u << 28) ? 5u : 6u;
}

// its octet j (h: 0x80 for the H-bit form, ORed into octet 0)
__device__ __forceinline__ uint32_t str_poctet(uint32_t p, uint32_t plen, uint32_t j, uint32_t h) {
    if (j == 0) return h | (p < 127u ? p : 127u);
    const uint32_t g = ((p - 127u) >> (7u * (j - 1u))) & 127u;
    return j + 1u < plen ? g | 128u : g;
}

// A representation of `total` bytes for an input of `len` bytes under policy `pol` (0..3): the prefix length
// (0: verbatim), and whether the payload is the input's own bytes (raw, verbatim) or its Huffman coding.
__device__ __forceinline__ bool str_form(uint32_t total, uint32_t len, uint32_t pol, uint32_t& plen) {
    if (pol == HPK_STR_VERBATIM) {
        plen = 0;
        return true;
    }
    // the k with plen(total - k) == k: total = plen(p) + p has one solution
    uint32_t k = 1;
    while (k < 6u && str_plen(total - k) != k) ++k;
    plen = k;
    const uint32_t p = total - k;
    return !(pol == HPK_STR_HUFFMAN || (pol == HPK_STR_AUTO && p < len));
}

// ---------------------------------------------------------------------------------------------
// The form step of the length pass, elementwise after hpk_enclen: out_len[i] holds literal i's Huffman bytes
// (0 with bad offsets) and becomes the representation's length. A literal with bad offsets or a policy above 3
// is void: length 0, HPK_BAD_OFFSETS, the sticky flag.
struct StrLenArgs {
    const uint32_t* in_off;
    uint32_t n, in_cap;
    const uint8_t* policy;  // may be null: all HPK_STR_AUTO
    uint32_t* out_len;
    uint8_t* status;  // may be null
    uint32_t* err;
};

__global__ __launch_bounds__(256) void hpk_strlen_form(StrLenArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t s = a.in_off[i], e = a.in_off[i + 1];
    const uint32_t pol = a.policy ? a.policy[i] : (uint32_t)HPK_STR_AUTO;
    const bool ok = s <= e && e <= a.in_cap && pol <= (uint32_t)HPK_STR_VERBATIM;
    uint64_t total = 0;
    if (ok) {
        const uint32_t len = e - s, h = a.out_len[i];
        if (pol == HPK_STR_VERBATIM) {
            total = len;
        } else {
            const bool huff = pol == HPK_STR_HUFFMAN || (pol == HPK_STR_AUTO && h < len);
            const uint32_t p = huff ? h : len;
            total = (uint64_t)p + str_plen(p);
        }
    } else {
        *a.err = 1u;
    }
    a.out_len[i] = total > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)total;  // (such a batch's total passes HPK_MAX_OFFSET)
    if (a.status) a.status[i] = (uint8_t)(ok ? HPK_OK : HPK_BAD_OFFSETS);
}

// ---------------------------------------------------------------------------------------------
// The emit step: hpk_encode2's packed instantiation (hpk_encode_kernel.h, whose comments explain the tile, the
// start map, the two passes and the write-back) with a prefix in front of every literal's codes and raw
// payloads. What differs:
//   * a literal's region [out_off[i], out_off[i+1]) is its whole representation; its codes start plen bytes
//     into it (cst, beside ooff), and the per-literal thread ORs the prefix octets into the image after pass 2;
//   * a raw or verbatim literal's bytes go through the image as 8-bit codes of themselves: pass 2 picks
//     (byte, 8) instead of the table's (code, length) per run, and the carry into a thread whose first byte
//     continues a raw literal is 8 bits per byte since the literal's start (pass 1's scan sums Huffman lengths);
//   * a literal that fits no tile: a raw or verbatim one is copied by the whole workgroup, a Huffman one is
//     coded by one lane, the prefix in front of either;
//   * only the packed arms exist: exact regions, the branch-free pass 2, every image chunk live.
struct StrArgs {
    const uint8_t* in_blob;
    const uint32_t* in_off;
    uint32_t n;
    const uint8_t* policy;  // may be null: all HPK_STR_AUTO
    uint8_t* out_blob;
    const uint32_t* out_off;
    uint32_t* out_len;
    uint8_t* status;
    const uint32_t* codes;  // [0,257): right-aligned code, [257,514): length
    const uint8_t* in_base;  // 16-byte aligned bases and the blobs' misalignment
    uint32_t in_mis;
    uint8_t* out_base;
    uint32_t out_mis;
    uint32_t in_cap, out_cap;
    const unsigned long long* void_all;  // the length scan's verdict
    unsigned long long* prof;            // diagnostic build: cycles per kernel phase (kProf), hpk_encode2's phases
};

// threads per workgroup, bytes of the LDS image, literals per tile (32 input bytes per thread per tile); two
// workgroups per CU as hpk_encode2: the image is 48 KiB, not 56, to make room for cst
constexpr int kStrEB = 512, kStrEO = 48 * 1024, kStrEQ = 1024;
constexpr uint32_t kCstRaw = 0x80000000u;

template <int kEB, int kEO, int kEQ, int kP = 0>
struct StrLds {
    uint32_t img[kEO / 4 + kEPh];  // the tile's output span, big-endian dwords; then the phantom dwords
    uint32_t ioff[kEQ + 3];        // input offsets of the tile's literals, relative to the tile base (+ sentinel)
    uint32_t ooff[kEQ + 2];        // output offsets (the representations' starts), relative to the image base
    uint32_t cst[kEQ + 2];         // where the literal's payload starts (ooff + plen); kCstRaw: its own bytes
    uint32_t bits[kEQ];            // payload bits per literal (set by the thread holding its last byte)
    uint2 tab[256];                // (code, length)
    uint32_t code1[256];           // one-lane path: codes
    uint8_t len1[256];             // pass 1 and the one-lane path: lengths
    uint32_t wf[16], wv[16], wl[16];
    uint32_t smap[kEB + 1];
    uint32_t slast[kEB + 1];
    uint32_t ctr[4];  // [0] literals in the tile, [1] bad offsets seen, [3] the window's first bad literal
    uint32_t split[2 * hpksplit::kMaxRounds];
    unsigned long long prof[kP ? kEB / 64 : 1][12];  // diagnostic build (kProf): per-wave phase cycles
};

// One literal, one lane, global memory: the prefix, then the payload copied or coded; bytes at or past the
// blob's capacity are not stored. (A Huffman literal above a tile, and the literals after a bad one.)
__device__ __forceinline__ void str_serial(const StrArgs& a, const uint32_t* code, const uint8_t* len, uint32_t i,
                                           uint32_t pol) {
    const uint32_t s = a.in_off[i], e = a.in_off[i + 1];
    const uint32_t o0 = a.out_off[i], total = a.out_off[i + 1] - o0;
    uint32_t plen;
    const bool raw = str_form(total, e - s, pol, plen);
    auto put = [&](uint32_t o, uint32_t b) {
        if (o0 + o < a.out_cap) a.out_blob[o0 + o] = (uint8_t)b;
    };
    for (uint32_t j = 0; j < plen; ++j) put(j, str_poctet(total - plen, plen, j, raw ? 0u : 0x80u));
    uint32_t o = plen;
    if (raw) {
        for (uint32_t p = s; p < e; ++p) put(o++, a.in_blob[p]);
        return;
    }
    uint64_t acc = 0;
    int nb = 0;
    for (uint32_t p = s; p < e; ++p) {
        const uint32_t b = a.in_blob[p];
        acc = (acc << len[b]) | code[b];
        nb += len[b];
        while (nb >= 8) {
            nb -= 8;
            put(o++, (uint32_t)(acc >> nb));
        }
    }
    if (nb) put(o, (uint32_t)((acc << (8 - nb)) | (0xFFu >> nb)));
}

template <int kEB, int kEO, int kEQ, int kProf = 0>
__global__ __launch_bounds__(kEB, 4) void hpk_encode_str(StrArgs a) {
    constexpr int kEBytes = 32;
    constexpr int kETile = kEB * kEBytes;
    constexpr int kEMeta = kEQ / kEB;
    static_assert(2 * sizeof(StrLds<kEB, kEO, kEQ, kProf>) <= 163840, "two workgroups per CU (160 KiB of LDS on gfx950)");
    static_assert(kEB <= 1024 && kEQ % kEB == 0 && kEO % 16 == 0, "geometry");
    __shared__ __attribute__((aligned(16))) StrLds<kEB, kEO, kEQ, kProf> S;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    if (*a.void_all) {  // (uniform) the total passes HPK_MAX_OFFSET: every literal is void, no byte is written
        for (uint32_t i = blockIdx.x * (uint32_t)kEB + tid; i < a.n; i += gridDim.x * (uint32_t)kEB) {
            a.out_len[i] = 0;
            a.status[i] = (uint8_t)HPK_BAD_OFFSETS;
        }
        return;
    }
    uint64_t tprev = kProf ? clock64() : 0;
    if (kProf && tid < (kEB / 64) * 12) (&S.prof[0][0])[tid] = 0;
    if (tid < 256) {
        const uint32_t c = a.codes[tid], l = a.codes[257 + tid];
        S.tab[tid] = make_uint2(c, l);
        S.code1[tid] = c;
        S.len1[tid] = (uint8_t)l;
    }
    {
        uint4* i16 = reinterpret_cast<uint4*>(S.img);
        for (uint32_t c = tid; c < (uint32_t)kEO / 16; c += kEB) i16[c] = make_uint4(0, 0, 0, 0);
    }
    if (tid < 4) S.ctr[tid] = 0;
    for (uint32_t w = tid; w <= (uint32_t)kEB; w += kEB) {
        S.smap[w] = 0;
        S.slast[w] = 0;
    }
    uint32_t BA, BB;
    hpksplit::split_by_bytes<kEB, 16>(a.in_off, a.n, S.split, BA, BB);  // (barriers: the clears are seen)
    EPROF(8);
    const uint32_t in_end = a.in_cap + a.in_mis;  // loads are clamped to the blob's last 16-byte chunk
    const uint32_t last16 = in_end ? (in_end - 1) >> 4 : 0;
    const uint4* g_in = reinterpret_cast<const uint4*>(a.in_base);
    uint4 ch[2] = {};
    uint32_t pi0[kEMeta], pi1[kEMeta], po0[kEMeta], po1[kEMeta], pp[kEMeta];
    auto prefetch = [&](uint32_t c, uint32_t base16) {
        const uint32_t cn = min((uint32_t)kEQ, BB - c);
#pragma unroll
        for (int r = 0; r < 2; ++r) ch[r] = g_in[min((base16 >> 4) + 2u * tid + (uint32_t)r, last16)];
#pragma unroll
        for (int r = 0; r < kEMeta; ++r) {
            const uint32_t t = min(tid + (uint32_t)kEB * r, cn - 1u);
            pi0[r] = a.in_off[c + t];
            pi1[r] = a.in_off[c + t + 1];
            po0[r] = a.out_off[c + t];
            po1[r] = a.out_off[c + t + 1];
            pp[r] = a.policy ? a.policy[c + t] : (uint32_t)HPK_STR_AUTO;
        }
    };
    uint32_t cur = BA;
    uint32_t gin = 0, gout = 0;  // the tile's input / output start (base-relative: + mis)
    const uint32_t range_end = BB;  // (BB is pulled in to the range's first void literal, once seen)
    if (cur < BB) {
        gin = a.in_off[cur] + a.in_mis;
        gout = a.out_off[cur] + a.out_mis;
        prefetch(cur, gin & ~15u);
    }
    while (cur < BB) {  // block-uniform
        const uint32_t cntl = min((uint32_t)kEQ, BB - cur);
        const uint32_t base16 = gin & ~15u, ob16 = gout & ~15u;
        EPROF(7);
        lds_barrier_e();  // the previous tile's image is out
        EPROF(11);
        auto good = [&](int r) { return pi0[r] <= pi1[r] && pi1[r] <= a.in_cap && pp[r] <= (uint32_t)HPK_STR_VERBATIM; };
        uint32_t kw = 0;
        bool bad = false;
#pragma unroll
        for (int r = 0; r < kEMeta; ++r) {
            const uint32_t t = tid + (uint32_t)kEB * r;
            bad |= t < cntl && !good(r);
        }
#pragma unroll
        for (int r = 0; r < kEMeta; ++r) {
            const uint32_t t = tid + (uint32_t)kEB * r;
            bool fits = false;
            const uint32_t i0 = pi0[r] + a.in_mis, i1 = pi1[r] + a.in_mis;
            const uint32_t o0 = po0[r] + a.out_mis, o1 = po1[r] + a.out_mis;
            if (t < cntl && !bad) fits = i1 - base16 <= (uint32_t)kETile && o1 - ob16 <= (uint32_t)kEO;
            if (fits) {
                uint32_t plen;
                const bool raw = str_form(o1 - o0, i1 - i0, pp[r], plen);
                S.ioff[t] = i0 - base16;
                S.ooff[t] = o0 - ob16;
                S.cst[t] = (o0 - ob16 + plen) | (raw ? kCstRaw : 0u);
                S.ioff[t + 1] = i1 - base16;  // (the same value literal t + 1 writes)
                S.ooff[t + 1] = o1 - ob16;
                S.bits[t] = 0;
                if (i1 > i0) {
                    const uint32_t x = i0 - base16;
                    atomicOr(&S.smap[x >> 5], 1u << (x & 31u));
                    atomicMax(&S.slast[x >> 5], t + 1u);
                }
            }
            kw += (uint32_t)__popcll(__ballot(fits));
        }
        if (lane == 0 && kw) atomicAdd(&S.ctr[0], kw);
        if (__any(bad) && lane == 0) S.ctr[1] = 1u;
        const uint4 chc0 = ch[0], chc1 = ch[1];
        EPROF(1);
        lds_barrier_e();
        EPROF(11);
        if (S.ctr[1]) {  // a void literal in the window (block-uniform): the literals before it are encoded by
            // tiles, the range's rest one literal per lane after the loop (hpk_encode2's rare path)
            if (tid == 0) S.ctr[3] = cntl;
            lds_barrier_e();
#pragma unroll
            for (int r = 0; r < kEMeta; ++r) {
                const uint32_t t = tid + (uint32_t)kEB * r;
                if (t < cntl && !good(r)) atomicMin(&S.ctr[3], t);
            }
            lds_barrier_e();
            if (tid == 0) {
                S.ctr[0] = 0;
                S.ctr[1] = 0;
            }
            for (uint32_t w = tid; w <= (uint32_t)kEB; w += kEB) {
                S.smap[w] = 0;
                S.slast[w] = 0;
            }
            BB = cur + S.ctr[3];
            continue;
        }
        const uint32_t k = S.ctr[0];
        if (tid == 0) S.ioff[k + 1] = 0xFFFFFFFFu;  // pass 2's literal search stops at the phantom literal k
        if (k == 0) {  // literal `cur` alone exceeds a tile
            const uint32_t s = a.in_off[cur], len = a.in_off[cur + 1] - s;
            const uint32_t o0 = a.out_off[cur], total = a.out_off[cur + 1] - o0;
            const uint32_t pol = a.policy ? a.policy[cur] : (uint32_t)HPK_STR_AUTO;
            uint32_t plen;
            if (str_form(total, len, pol, plen)) {  // its own bytes: the whole workgroup copies them
                if (tid < plen && o0 + tid < a.out_cap) a.out_blob[o0 + tid] = (uint8_t)str_poctet(len, plen, tid, 0u);
                const uint32_t room = a.out_cap > o0 + plen ? a.out_cap - (o0 + plen) : 0u;
                const uint8_t* src = a.in_blob + s;
                uint8_t* dst = a.out_blob + o0 + plen;
                for (uint32_t x = tid; x < min(len, room); x += kEB) dst[x] = src[x];
            } else if (tid == 0) {
                str_serial(a, S.code1, S.len1, cur, pol);
            }
            cur += 1;
            if (cur < BB) {
                gin = a.in_off[cur] + a.in_mis;
                gout = a.out_off[cur] + a.out_mis;
                prefetch(cur, gin & ~15u);
            }
            continue;
        }
        const uint32_t cur_n = cur + k;
        const uint32_t gin_n = S.ioff[k] + base16, gout_n = S.ooff[k] + ob16;
        if (cur_n < BB) prefetch(cur_n, gin_n & ~15u);
        const uint32_t xb = S.ioff[0], xe = S.ioff[k];  // the tile's input bytes [xb, xe)
        const uint32_t x0 = max(tid * (uint32_t)kEBytes, xb), x1 = min(tid * (uint32_t)kEBytes + kEBytes, xe);
        const bool any = x0 < x1;
        const uint32_t xt = tid * (uint32_t)kEBytes;
        const uint32_t sm = S.smap[tid], snext = S.smap[tid + 1], sl = S.slast[tid];
        const uint32_t wd[8] = {chc0.x, chc0.y, chc0.z, chc0.w, chc1.x, chc1.y, chc1.z, chc1.w};
        uint32_t bm = 0, vm = 0;
        bool f0 = false;         // the thread's first byte starts a literal
        bool ends_here = false;  // the thread's last literal ends at its last byte
        if (any) {
            vm = (uint32_t)(((1ull << (x1 - x0)) - 1ull) << (x0 - xt));
            f0 = (sm >> (x0 - xt)) & 1u;
            bm = sm & vm & ~(1u << (x0 - xt));
            ends_here = x1 == xe || (snext & 1u);
        }
        const uint32_t bm2 = bm | (any && x0 > xt ? 1u << (x0 - xt) : 0u) |
                             (any && x1 < xt + (uint32_t)kEBytes ? 1u << (x1 - xt) : 0u);
        EPROF(2);
        // pass 1: the Huffman code lengths of the owned bytes from the last literal start on (a raw literal's
        // bytes are summed too; its carry is taken from the offsets below)
        const uint32_t f = (f0 || bm) ? 1u : 0u;
        const uint32_t cm = bm ? vm & ~((1u << (31u - __builtin_clz(bm))) - 1u) : vm;
        uint32_t v = 0;
#pragma unroll 1
        for (uint32_t g = 0; g < (uint32_t)kEBytes / 8u; ++g) {
            const uint32_t lo8 = g == 0 ? wd[0] : g == 1 ? wd[2] : g == 2 ? wd[4] : wd[6];
            const uint32_t hi8 = g == 0 ? wd[1] : g == 1 ? wd[3] : g == 2 ? wd[5] : wd[7];
            const uint32_t cm8 = cm >> (8u * g);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t ln = S.len1[((j < 4 ? lo8 : hi8) >> (8 * (j & 3))) & 0xFFu];
                v += ln & (uint32_t)__builtin_amdgcn_sbfe((int)cm8, j, 1);
            }
        }
        EPROF(3);
        uint32_t fi = f, vi = v, Li = sl;
        wave_seg_scan(fi, vi, Li, lane);
        if (lane == 63) {
            S.wf[wv] = fi;
            S.wv[wv] = vi;
            S.wl[wv] = Li;
        }
        EPROF(4);
        lds_barrier_e();
        EPROF(11);
        uint32_t cw = 0, cl = 0;
#pragma unroll
        for (uint32_t j = 0; j < (uint32_t)kEB / 64u - 1u; ++j) {
            const uint32_t wf = S.wf[j], wvv = S.wv[j], wl = S.wl[j];
            if (j < wv) {
                cw = wf ? wvv : cw + wvv;
                cl = max(cl, wl);
            }
        }
        const uint32_t ef = dpp_e<0x138>(fi), ev = dpp_e<0x138>(vi), el = dpp_e<0x138>(Li);  // wave_shr:1
        uint32_t carry = ef ? ev : cw + ev;
        if (tid == 0) {
            S.ctr[0] = 0;
            S.ctr[1] = 0;
        }
        for (uint32_t w = tid; w <= (uint32_t)kEB; w += kEB) {
            S.smap[w] = 0;
            S.slast[w] = 0;
        }
        const uint32_t lx = max(cl, el);  // 1 + the last non-empty literal starting before byte xt
        uint32_t li = 0;
        if (any) {
            if (f0) {
                li = lx;
                while (S.ioff[li + 1] <= x0) ++li;
            } else {
                li = lx - 1u;
            }
        }
        EPROF(4);
        {  // pass 2 (hpk_encode2's branch-free one). (A wave-uniform flag per 2 KiB of the tile, "a raw literal
            // touches these bytes", choosing between this loop and one without the selects, measured slower:
            // config 3 573-575 vs 549-553 us)
            uint32_t lj = any && x0 > xt ? li - 1u : li;
            uint32_t nc = S.cst[lj + 1u], nx = S.ioff[lj + 2u];
            bool ph = !any || x0 > xt;  // in a phantom run
            const uint32_t qph = (uint32_t)(kEO / 4 + (tid & 31u)) * 32u;
            const uint32_t c0 = ph ? 0u : S.cst[li];
            bool raw = (c0 & kCstRaw) != 0u;
            if (raw && !f0) carry = 8u * (x0 - S.ioff[li]);
            uint32_t qs = ph ? qph : (c0 & ~kCstRaw) * 8u;  // the run's literal's first payload bit
            const uint32_t q = ph ? qph : qs + (f0 ? 0u : carry);
            uint32_t dq = q >> 5, n = q & 31u;
            uint64_t acc = 0;
#pragma unroll 1
            for (uint32_t g = 0; g < (uint32_t)kEBytes / 8u; ++g) {
                const uint32_t lo8 = g == 0 ? wd[0] : g == 1 ? wd[2] : g == 2 ? wd[4] : wd[6];
                const uint32_t hi8 = g == 0 ? wd[1] : g == 1 ? wd[3] : g == 2 ? wd[5] : wd[7];
                const uint32_t bm8 = bm2 >> (8u * g);
                uint32_t by[8];
                uint2 tb[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    by[j] = ((j < 4 ? lo8 : hi8) >> (8 * (j & 3))) & 0xFFu;
                    tb[j] = S.tab[by[j]];
                }
                auto start = [&](int j) {  // a run starts at byte j: close the previous one
                    if (n) atomicOr(&S.img[dq], (uint32_t)(acc << (32u - n)));
                    if (!ph) S.bits[lj] = dq * 32u + n - qs;
                    const uint32_t x = xt + 8u * g + (uint32_t)j;
                    uint32_t cs;
                    if (nx > x) {
                        ++lj;
                        cs = nc;
                    } else {
                        while (S.ioff[lj + 1] <= x) ++lj;  // (empty literals between: bits stay 0)
                        cs = S.cst[lj];
                    }
                    ph = lj >= k;  // the tile's end: the rest is a phantom
                    raw = !ph && (cs & kCstRaw) != 0u;
                    qs = ph ? qph : (cs & ~kCstRaw) * 8u;
                    nc = S.cst[lj + 1u];
                    nx = S.ioff[lj + 2u];
                    dq = qs >> 5;
                    n = qs & 31u;
                    acc = 0;
                };
                auto put = [&](uint2 t2, uint32_t b) {
                    const uint32_t c = raw ? b : t2.x, l = raw ? 8u : t2.y;
                    acc = (acc << l) | c;
                    n += l;  // 5 <= n < 62
                    const bool full = n >= 32u;
                    atomicOr(&S.img[dq], (uint32_t)((acc << (64u - n)) >> 32));
                    dq += full ? 1u : 0u;
                    n &= 31u;
                };
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if ((bm8 >> j) & 1u) start(j);
                    put(tb[j], by[j]);
                }
            }
            if (any && !ph) {
                if (n) atomicOr(&S.img[dq], (uint32_t)(acc << (32u - n)));
                if (ends_here) S.bits[lj] = dq * 32u + n - qs;
            }
        }
        EPROF(5);
        lds_barrier_e();
        EPROF(11);
        // per literal: the prefix octets, the EOS padding
#pragma unroll
        for (int r = 0; r < kEMeta; ++r) {
            const uint32_t t = tid + (uint32_t)kEB * r;
            if (t < k) {
                const uint32_t o = S.ooff[t], c = S.cst[t], cs = c & ~kCstRaw;
                const uint32_t plen = cs - o, p = S.ooff[t + 1] - cs;
                for (uint32_t j = 0; j < plen; ++j)
                    img_or(S.img, (o + j) * 8u, str_poctet(p, plen, j, (c & kCstRaw) ? 0u : 0x80u), 8u);
                const uint32_t bits = S.bits[t];
                if (bits & 7u) {
                    const uint32_t pad = 8u - (bits & 7u);
                    img_or(S.img, cs * 8u + bits, (1u << pad) - 1u, pad);
                }
            }
        }
        EPROF(6);
        lds_barrier_e();
        EPROF(11);
        {  // write the image back: bytes [G0, G1) of the image (relative to ob16)
            const uint32_t G0 = S.ooff[0], G1 = S.ooff[k];
            const uint32_t c1 = (G1 + 15u) >> 4;
            const uint4* i16 = reinterpret_cast<const uint4*>(S.img);
            uint4* g16 = reinterpret_cast<uint4*>(a.out_base + ob16);
            uint4* m16 = reinterpret_cast<uint4*>(S.img);
            // the image bytes below the blob's capacity: [G0, Gs). Gs < G1 only in the one tile that crosses
            // the capacity and in the tiles past it: the bytes go out one by one, then the span is cleared
            const uint32_t room = a.out_cap + a.out_mis;
            const uint32_t Gs = room >= ob16 + G1 ? G1 : room > ob16 + G0 ? room - ob16 : G0;
            if (Gs < G1) {  // (block-uniform)
                for (uint32_t x = G0 + tid; x < Gs; x += kEB) {
                    const uint32_t w = S.img[x >> 2];
                    a.out_base[ob16 + x] = (uint8_t)(w >> (24u - 8u * (x & 3u)));
                }
                lds_barrier_e();
                for (uint32_t c = tid; c < c1; c += kEB) m16[c] = make_uint4(0, 0, 0, 0);
                cur = cur_n;
                gin = gin_n;
                gout = gout_n;
                continue;
            }
            for (uint32_t c = tid; c < c1; c += kEB) {
                if ((c << 4) >= G0 && (c << 4) + 16u <= G1) {
                    const uint4 w = i16[c];
                    g16[c] = make_uint4(__builtin_bswap32(w.x), __builtin_bswap32(w.y), __builtin_bswap32(w.z),
                                        __builtin_bswap32(w.w));
                    m16[c] = make_uint4(0, 0, 0, 0);
                }
            }
            if (tid < 32) {  // the partial chunks at the two ends, one byte per lane (lanes 16-31: the last chunk
                // when it is not also the first)
                const uint32_t g = tid < 16 || c1 < 2u ? 0u : (c1 - 1u) << 4;
                const bool partial = !(g >= G0 && g + 16u <= G1) && (tid < 16 ? c1 != 0u : c1 > 1u);
                const uint32_t x = g + (tid & 15u);
                if (partial && x >= G0 && x < G1) {
                    const uint32_t w = S.img[x >> 2];
                    a.out_base[ob16 + x] = (uint8_t)(w >> (24u - 8u * (x & 3u)));
                }
                if ((tid & 15u) == 0 && partial) m16[g >> 4] = make_uint4(0, 0, 0, 0);
            }
        }
        cur = cur_n;
        gin = gin_n;
        gout = gout_n;
    }
    // from the range's first void literal on: the length pass has voided exactly the void ones and counted the
    // others, which are written one per lane (they may overlap in the input; a lane writes its own bytes only)
    for (uint32_t i = BB + tid; i < range_end; i += kEB) {
        const uint32_t s = a.in_off[i], e = a.in_off[i + 1];
        const uint32_t pol = a.policy ? a.policy[i] : (uint32_t)HPK_STR_AUTO;
        if (s <= e && e <= a.in_cap && pol <= (uint32_t)HPK_STR_VERBATIM) str_serial(a, S.code1, S.len1, i, pol);
    }
    if (kProf) {
        __syncthreads();
        if (tid < (kEB / 64) * 12) atomicAdd(&a.prof[tid % 12], S.prof[tid / 12][tid % 12]);
    }
}

}  // namespace

// out_len (hpk_enclen's Huffman byte counts) -> the representations' lengths, status if not null
int hpk_launch_strlen_form(hpk_ctx* c, uint32_t in_cap, const uint32_t* in_off, uint32_t n, const uint8_t* policy,
                           uint32_t* out_len, uint8_t* status) {
    const StrLenArgs a{in_off, n, in_cap, policy, out_len, status, c->d_err};
    hipLaunchKernelGGL(hpk_strlen_form, dim3((n + 255u) / 256u), dim3(256), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}

// The emit into b.out_off's exact regions; void_all: the length scan's verdict on the total.
int hpk_launch_encode_strings(hpk_ctx* c, const hpk_batch& b, const uint8_t* policy, const unsigned long long* void_all) {
    const auto in = split16(b.in_blob);
    const auto out = split16(b.out_blob);
    StrArgs a{b.in_blob,  b.in_off, b.n,    policy,   b.out_blob, b.out_off, b.out_len, b.status,
              c->d_codes, in.base,  in.mis, out.base, out.mis,    b.in_cap,  b.out_cap, void_all, nullptr};
    // the packed encode's grid: two workgroups per CU (the small-call mode's CUs left out), at least kProdPerWg
    // literals each
    uint64_t blocks = ((uint64_t)b.n + kProdPerWg - 1u) / kProdPerWg;
    const uint64_t cus = (uint64_t)c->num_cu - (c->sm_launched && c->sm_max ? (uint64_t)c->sm_wgs : 0u);
    if (blocks > cus * 2u) blocks = cus * 2u;
    if (blocks < 1) blocks = 1;
#ifdef HPK_DIAG
    const char* w = getenv("HPK_ENCODE_CFG");
    if (w && atoi(w) == 9) {  // with per-phase cycle counters (hpk_debug_encode_prof, as the packed encode's)
        if (!hpk_g_eprof) HIP_TRY(hipMalloc(&hpk_g_eprof, 16 * sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(hpk_g_eprof, 0, 16 * sizeof(unsigned long long), c->stream));
        a.prof = hpk_g_eprof;
        hipLaunchKernelGGL((hpk_encode_str<kStrEB, kStrEO, kStrEQ, 1>), dim3((uint32_t)blocks), dim3(kStrEB), 0, c->stream,
                           a);
        HIP_TRY(hipGetLastError());
        return HPK_E_OK;
    }
#endif
    hipLaunchKernelGGL((hpk_encode_str<kStrEB, kStrEO, kStrEQ>), dim3((uint32_t)blocks), dim3(kStrEB), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}

extern "C" int hpk_test_strings_geometry(uint32_t* tile_bytes, uint32_t* image_bytes, uint32_t* tile_literals,
                                         uint32_t* one_wg_literals) {
    if (!tile_bytes || !image_bytes || !tile_literals || !one_wg_literals) return HPK_E_INVAL;
    *tile_bytes = kStrEB * 32;
    *image_bytes = kStrEO;
    *tile_literals = kStrEQ;
    *one_wg_literals = kProdPerWg;
    return HPK_E_OK;
}
