// hpk_decode.hip — gfx950 batched Huffman literal decode (the hot path).
//
// Replaces, for a batch of literals at once, the Huffman branch of decode_string
// (crates/loona-hpack/src/decoder.rs:143-157) i.e. HuffmanDecoder::decode
// (crates/loona-hpack/src/huffman.rs:95-161), with identical results per literal: decoded bytes,
// and status Ok / PaddingTooLarge / InvalidPadding / EOSInString with the reference's precedence.
//
// Two kernels, identical results (tests/test_gpu.py runs every case through both):
//   * hpk_decode_wave (v25, hpk_wave.h), for every batch: every wave of a 1024-thread workgroup
//     decodes its own fills of <= 128 literals (two per lane, longest with shortest) out of its own
//     LDS window into its own LDS image, with no barrier between fills, so the waves' memory traffic
//     and setup overlap each other's decoding; the workgroup's range is handed out in chunks;
//   * hpk_decode12 (v24, hpk_fill.h), only when forced (hpk_ctx_set_decode_kernel(HPK_DECODE_FILL)):
//     one workgroup-wide fill at a time per CU (40 KiB window, 77 KiB image, 2048-literal
//     longest-first queue), the next fill's loads in flight during the decode, the previous image
//     written back around it.
// Both use the same lane walk (hpk_walk.h): a step is two lookups in the two-symbol table (13 index
// bits in the wave kernel since v39, 12 in the workgroup-fill and the small-call kernel), each decoding
// up to two codes within the index bits, from a 32-bit window made by ONE v_alignbit
// out of a register-held dword pair; a longer code (or EOS) takes one leading-ones lookup. Bits past
// a literal's end are not masked: a code that runs past the end is, by prefix-freeness, longer than
// what is left whatever follows, so the walk stops exactly where huffman.rs's bit iterator stops
// matching; only the final padding check (huffman.rs:128-160) looks at the residual bits. Literals
// of >= 64 encoded bytes go to the long-literal phase (hpk_long.h), one lane each streaming from
// HBM, after the fills; a literal whose output region is below hpk_decoded_bound is decoded code by
// code with a capacity check per byte (HPK_OUTPUT_OVERFLOW).
#include <stdlib.h>

#include <chrono>

#include "hpk_fill.h"
#include "hpk_wave.h"
#include "hpk_persist.h"

using namespace hpkdec;

// Workgroup-fill kernel (v24, hpk_fill.h): 16 waves (one 1024-thread workgroup) per CU; per
// fill a 40 KiB input window, a 77 KiB output image and a 2048-entry longest-first queue, plus the
// 16 KiB two-symbol table; lanes check for a finished literal every 2 steps.
constexpr int kWaves = 16, kW = 40960, kO = 79104, kQ = 2048, kRefillN = 2;
// long-literal phase (hpk_long.h, both kernels): literals of >= HPK_LONG_MIN encoded bytes, those of
// >= HPK_LONG_BIG first (longest-first, roughly)
#ifndef HPK_LONG_MIN
#define HPK_LONG_MIN 64
#endif
#ifndef HPK_LONG_BIG
#define HPK_LONG_BIG 1024
#endif
using Geo = Geo12<kWaves, kW, kO, kQ>;
// Wave-fill kernel (v25, hpk_wave.h): per wave a 3,008-byte window and a 5,040-byte image (v39: 8,048 bytes
// per wave beside the 13-bit table; until v38 3,072 + 5,888, the image's last 256 the dummy slots), the
// workgroup's range handed out in chunks of 224 literals; it runs every batch (since round 6; it had taken
// those of >= 4M literals: config 2 40.3-40.8 vs 47.1-47.3 us for the workgroup-fill kernel, 1k-literal
// synchronous calls 21.5 vs 24.4 us) unless the context forces the workgroup-fill kernel
// (hpk_ctx_set_decode_kernel)
#ifndef HPK_WAVE_WIN
#define HPK_WAVE_WIN 3008  // (config 5: 2880 696.0-701.9, 3008 681.7-691.0, 3136 761.3-767.5 us: a fourth window round)
#endif
#ifndef HPK_WAVE_IMG
#define HPK_WAVE_IMG (8048 - HPK_WAVE_WIN)
#endif
constexpr int kWaveWin = HPK_WAVE_WIN, kWaveImg = HPK_WAVE_IMG;
#ifndef HPK_WAVE_CHUNK
#define HPK_WAVE_CHUNK 224u  // least literals per chunk claim
#endif
// (the waves claim their chunks by guided self-scheduling: kGuided 1, hpk_wave.h)
#define WAVE_KERNEL(m) hpk_decode_wave<m, kWaveWin, kWaveImg, HPK_WAVE_CHUNK, 1>
// (round 6) batches below HPK_WAVE_GUIDED_MIN literals hand their workgroups' ranges out in fixed chunks of
// about one fill (config 2 with 104-literal chunks: 43.7-43.9 us against 51.1 guided, 44.1-45.0 static, 46.9
// for the workgroup-fill kernel; with the overlapped start, hpk_wave.h, and 96-literal chunks 40.3-40.6)
#ifndef HPK_WAVE_GUIDED_MIN
#define HPK_WAVE_GUIDED_MIN 4000000u
#endif
#ifndef HPK_WAVE_SMALL_CHUNK
#define HPK_WAVE_SMALL_CHUNK 96u  // (config 2: 88 43.1-43.5, 92 40.5-41.0, 96 40.3-40.6, 100 42.4-43.3, 104 43.3-43.9 us;
                                  // v39, fills of ~108 literals: 92 36.5-37.0, 96 36.4-37.8, 100 38.1-38.4)
#endif
#define WAVE_KERNEL_SMALL(m) hpk_decode_wave<m, kWaveWin, kWaveImg, HPK_WAVE_SMALL_CHUNK, 2>
#define DEC_KERNEL(m) hpk_decode12<m, kWaves, kW, kO, kQ, kRefillN>

#ifdef HPK_DIAG
// Diagnostic build (libhpk_diag.so, `make diag`; never the product library): HPK_DEBUG_MODE selects
// 1 no decode, 2 no output stores, 3 per-wave stamps (16 x u64 per wave, hpk_debug_stamps),
// 4 every store bounds-checked (fill kernel, hpk_debug_check), 5 per-wave counters of the long-literal
// phase, 8-10 LDS conflict attribution (wave kernel, lit12_body's kDup: the table
// reads / the window read / the byte stores issued twice).
static int g_debug_mode = -1;
static unsigned long long* g_dbg = nullptr;
static size_t g_dbg_n = 0;

// a.dbg for a launch that writes `need` u64 entries (grow-only), zeroed on the stream if asked
static int dbg_buffer(hpk_ctx* c, DecodeArgs& a, size_t need, bool zero) {
    if (need > g_dbg_n) {
        (void)hipFree(g_dbg);
        HIP_TRY(hipMalloc(&g_dbg, need * 8));
        g_dbg_n = need;
    }
    if (zero) HIP_TRY(hipMemsetAsync(g_dbg, 0, need * 8, c->stream));
    a.dbg = g_dbg;
    return HPK_E_OK;
}

extern "C" int hpk_debug_check(unsigned long long* host8) {
    return hipMemcpyFromSymbol(host8, HIP_SYMBOL(g_chk), 8 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}

extern "C" int hpk_debug_stamps(unsigned long long* host, size_t cap_entries) {
    if (!g_dbg) return 0;
    size_t n = g_dbg_n < cap_entries ? g_dbg_n : cap_entries;
    if (hipMemcpy(host, g_dbg, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int)n;
}
#endif

static void decode_args(hpk_ctx* c, const hpk_batch& b, DecodeArgs& a) {
    const auto in = split16(b.in_blob);
    const auto out = split16(b.out_blob);
    a.in_base = in.base;
    a.in_mis = in.mis;
    a.in_off = b.in_off;
    a.n = b.n;
    a.out_base = out.base;
    a.out_mis = out.mis;
    a.out_off = b.out_off;
    a.out_len = b.out_len;
    a.status = b.status;
    a.lo = c->d_lo;
    a.lut2 = c->d_lut2;
    a.lut3 = c->d_lut3;
    a.lut13 = c->d_lut13;
    a.dbg = nullptr;
    a.in_cap = b.in_cap;
    a.out_cap = b.out_cap;
    a.err = c->d_err;
    a.lit_out = b.out_off;
    a.co_off = nullptr;
    a.cursor = nullptr;
}

// one workgroup per CU; fewer when the batch is small (>= ~64 literals or ~32 KiB of input per
// workgroup: a batch of a few huge literals gets one workgroup each, hpk_huge.h)
static uint32_t decode_blocks(hpk_ctx* c, const hpk_batch& b) {
    uint64_t blocks = ((uint64_t)b.n + 63) / 64;
    if (blocks < ((uint64_t)b.in_cap + 32767) / 32768) blocks = ((uint64_t)b.in_cap + 32767) / 32768;
    if (blocks > (uint64_t)b.n) blocks = (uint64_t)b.n;
    // (the small-call mode's persistent workgroups hold sm_wgs CUs: a one-per-CU grid leaves them out, or its
    // last workgroups would wait for a CU the whole time)
    const uint64_t cus = (uint64_t)c->num_cu - (c->sm_launched && c->sm_max ? (uint64_t)c->sm_wgs : 0u);
    if (blocks > cus) blocks = cus;
    if (blocks < 1) blocks = 1;
    return (uint32_t)blocks;
}

// ---- the small-call mode (hpk_persist.h) ----
constexpr int kPersistThreads = 256;

static int persist_launch(hpk_ctx* c, uint32_t base) {
    auto* h = static_cast<PersistCtl*>(c->h_sm);
    if (c->sm_launched) HIP_TRY(hipStreamSynchronize(c->sm_stream));  // (the previous kernel has exited)
    __atomic_store_n(&h->stop, 0u, __ATOMIC_RELAXED);
    __atomic_store_n(&h->done, base, __ATOMIC_RELAXED);
    __atomic_store_n(&h->declined, 0u, __ATOMIC_RELAXED);
    __atomic_store_n(&h->alive, 1u, __ATOMIC_RELEASE);
    const uint32_t init[4] = {0u, base, 0u, 0u};
    HIP_TRY(hipMemcpyAsync(c->d_sm_dev, init, sizeof init, hipMemcpyHostToDevice, c->sm_stream));
    PersistArgs a{static_cast<PersistCtl*>(c->d_sm), c->d_sm_dev, c->d_lut3, c->d_lo, base, c->sm_idle_ms * 100000u};
    hipLaunchKernelGGL(hpk_persist<kPersistThreads>, dim3((uint32_t)c->sm_wgs), dim3(kPersistThreads), 0, c->sm_stream, a);
    HIP_TRY(hipGetLastError());
    c->sm_launched = true;
    return HPK_E_OK;
}

int hpk_persist_start(hpk_ctx* c) { return persist_launch(c, c->sm_req); }

// The request number after k. Two values are never issued: kPersistExit, which the kernel reads as its exit
// command (it would leave, be launched again, read the same request and leave again until the call's deadline),
// and 0, the declined word's value after a launch (the request's last workgroup would report a good batch as
// declined). A launch's base is the last number issued (or 0 before the first), so it is never kPersistExit.
static uint32_t persist_next(uint32_t k) {
    do k += 1u;
    while (k == kPersistExit || k == 0u);
    return k;
}

extern "C" uint64_t hpk_test_small_calls(const hpk_ctx* c) { return c ? c->sm_calls : 0u; }

extern "C" int hpk_test_persist_geometry(uint32_t* slot_max, uint32_t* slot_chunks, uint32_t* out_dwords, uint32_t* threads) {
    if (!slot_max || !slot_chunks || !out_dwords || !threads) return HPK_E_INVAL;
    *slot_max = kPersistSlotMax;
    *slot_chunks = kPersistSlotChunks;
    *out_dwords = kPersistOutDw;
    *threads = (uint32_t)kPersistThreads;
    return HPK_E_OK;
}

extern "C" int hpk_test_small_stamps(const hpk_ctx* c, uint32_t* out10) {
    if (!c || !c->h_sm || !out10) return HPK_E_INVAL;
    const auto* h = static_cast<const PersistCtl*>(c->h_sm);
    for (int k = 0; k < 6; ++k) out10[k] = __atomic_load_n(&h->ts[k], __ATOMIC_ACQUIRE);
    for (int k = 0; k < 4; ++k) out10[6 + k] = __atomic_load_n(&h->tl[k], __ATOMIC_ACQUIRE);
    return HPK_E_OK;
}

int hpk_persist_stop(hpk_ctx* c) {
    if (!c->sm_launched) return HPK_E_OK;
    auto* h = static_cast<PersistCtl*>(c->h_sm);
    __atomic_store_n(&h->stop, 1u, __ATOMIC_RELEASE);
    HIP_TRY(hipStreamSynchronize(c->sm_stream));
    c->sm_launched = false;
    return HPK_E_OK;
}

extern "C" int hpk_test_small_set_request(hpk_ctx* c, uint32_t v) {
    if (!c || !c->h_sm || v == kPersistExit) return HPK_E_INVAL;  // (never issued, so never a launch's base either)
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = hpk_persist_stop(c)) return rc;
    c->sm_req = v;  // (the next call launches the kernel with this base)
    return HPK_E_OK;
}

int hpk_persist_call(hpk_ctx* c, const hpk_batch& b, bool* handled) {
    *handled = false;
    if (!c->sm_max || b.n > c->sm_max || b.n == 0) return HPK_E_OK;
    // the kernel does not follow the caller's stream order: the work queued there before this call (a
    // synchronous call waits for it anyway) is finished first
    if (hipStreamQuery(c->stream) != hipSuccess) HIP_TRY(hipStreamSynchronize(c->stream));
    auto* h = static_cast<PersistCtl*>(c->h_sm);
    if (!c->sm_launched || __atomic_load_n(&h->alive, __ATOMIC_ACQUIRE) == 0u)
        if (int rc = persist_launch(c, c->sm_req)) return rc;
    const auto in = split16(b.in_blob);
    const auto out = split16(b.out_blob);
    h->in_base = in.base;
    h->out_base = out.base;
    h->in_off = b.in_off;
    h->out_off = b.out_off;
    h->out_len = b.out_len;
    h->status = b.status;
    h->n = b.n;
    h->in_mis = in.mis;
    h->out_mis = out.mis;
    h->in_cap = b.in_cap;
    h->out_cap = b.out_cap;
    const uint32_t prev = c->sm_req, k = persist_next(prev);
    c->sm_req = k;
    __atomic_store_n(&h->req, k, __ATOMIC_RELEASE);
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0; __atomic_load_n(&h->done, __ATOMIC_ACQUIRE) != k; ++spins) {
        if (__atomic_load_n(&h->alive, __ATOMIC_ACQUIRE) == 0u) {  // it went idle just before the request
            if (int rc = persist_launch(c, prev)) return rc;
        }
        __builtin_ia32_pause();
        if ((spins & 4095u) == 4095u && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10))
            return hpk_set_err_msg("small-call mode: the persistent kernel did not answer", HPK_E_DEVICE);
    }
    *handled = __atomic_load_n(&h->declined, __ATOMIC_ACQUIRE) == 0u;  // (declined: bad offsets, the launch path's)
    c->sm_calls += *handled ? 1u : 0u;
    return HPK_E_OK;
}

// The compacted form: the wave-fill kernel's (each workgroup packs into its range's bound span, no device
// cursor: *wave = 1, out_off[n] is then the bound layout's end) unless the context forces the workgroup-fill
// kernel's (fills packed from the device cursor, *wave = 0); HPK_DECODE_AUTO selects the wave kernel for
// every batch, as the region form does
static bool wave_selected(const hpk_ctx* c) {
    return c->decode_kernel == HPK_DECODE_WAVE || c->decode_kernel == HPK_DECODE_AUTO;
}

bool hpk_compact_wave(const hpk_ctx* c, uint32_t) { return wave_selected(c); }

int hpk_launch_decode_compact(hpk_ctx* c, const hpk_batch& b, uint32_t* co_off, uint32_t* long_list, uint32_t* cursor,
                              bool wave) {
    DecodeArgs a;
    decode_args(c, b, a);
    a.lit_out = co_off;
    a.co_off = co_off;
    a.cursor = cursor;
    a.long_list = long_list;
    a.long_min = HPK_LONG_MIN;
    a.long_big = HPK_LONG_BIG;
    if (wave) {
        a.cursor = nullptr;  // (the huge phase takes a listed literal's region from co_off)
        hipLaunchKernelGGL((hpk_decode_wave<0, kWaveWin, kWaveImg, HPK_WAVE_CHUNK, 1, true>),
                           dim3(decode_blocks(c, b)), dim3(Geo::kBlock), 0, c->stream, a);
    } else {
        hipLaunchKernelGGL((hpk_decode12<0, kWaves, kW, kO, kQ, kRefillN, true>), dim3(decode_blocks(c, b)),
                           dim3(Geo::kBlock), 0, c->stream, a);
    }
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}

extern "C" int hpk_test_decode_geometry(int kind, uint32_t* out13) {
    if (!out13 || (kind != HPK_DECODE_FILL && kind != HPK_DECODE_WAVE)) return HPK_E_INVAL;
    using GW = GeoW<kWaveWin, kWaveImg, kWaveTab>;
    out13[0] = kind == HPK_DECODE_WAVE ? GW::kBlock : Geo::kBlock;
    out13[1] = HPK_HUGE_MIN;
    out13[2] = kHugeMax;
    out13[3] = kHugePieceMin;
    out13[4] = HPK_LONG_MIN;
    out13[5] = HPK_LONG_BIG;
    out13[6] = HPK_LONG_RING;
    out13[7] = HPK_LONG_CH;
    out13[8] = HPK_LONG_U;
    out13[9] = HPK_LONG_CLAIM;
    out13[10] = HPK_LONG_WAVES;
    out13[11] = HPK_LONG_OS;
    out13[12] = kind == HPK_DECODE_WAVE ? kWaveTab : 2;  // huge_phase / long_phase's kTab
    return HPK_E_OK;
}

int hpk_launch_decode(hpk_ctx* c, const hpk_batch& b, uint32_t* long_list) {
    DecodeArgs a;
    decode_args(c, b, a);
    a.long_list = long_list;
    a.long_min = HPK_LONG_MIN;
    a.long_big = HPK_LONG_BIG;
#ifdef HPK_DIAG
    if (const char* lm = getenv("HPK_LONG_MIN")) a.long_min = (uint32_t)atoi(lm);
    if (const char* lb = getenv("HPK_LONG_BIG")) a.long_big = (uint32_t)atoi(lb);
#endif
    const uint32_t blocks = decode_blocks(c, b);
    const dim3 grid(blocks), block(Geo::kBlock);
    bool wave = wave_selected(c);
#ifdef HPK_DIAG
    if (const char* wk = getenv("HPK_DECODE_KERNEL")) wave = wk[0] == 'w';  // "wave" / "fill" (A/B runs)
    if (g_debug_mode < 0) {
        const char* dm = getenv("HPK_DEBUG_MODE");
        g_debug_mode = dm ? atoi(dm) : 0;
    }
    // modes 3 and 5 write per-wave entries (16 each) into a.dbg; mode 5 adds to them, so they start zeroed
    if (g_debug_mode == 3 || g_debug_mode == 5) {
        const size_t waves = g_debug_mode == 3 ? kWaves : HPK_LONG_WAVES;
        if (int rc = dbg_buffer(c, a, (size_t)blocks * waves * 16, g_debug_mode == 5)) return rc;
    }
    // (every mode runs the kernel the product would: fixed chunks below HPK_WAVE_GUIDED_MIN literals)
#define WAVE_MODE(m)                                                                  \
    case m:                                                                           \
        if (b.n < HPK_WAVE_GUIDED_MIN)                                                \
            hipLaunchKernelGGL(WAVE_KERNEL_SMALL(m), grid, block, 0, c->stream, a);   \
        else                                                                          \
            hipLaunchKernelGGL(WAVE_KERNEL(m), grid, block, 0, c->stream, a);         \
        break;
#define FILL_MODE(m) \
    case m: hipLaunchKernelGGL(DEC_KERNEL(m), grid, block, 0, c->stream, a); break;
    if (wave) {
        switch (g_debug_mode) {
            WAVE_MODE(1) WAVE_MODE(2) WAVE_MODE(3) WAVE_MODE(5) WAVE_MODE(8) WAVE_MODE(9) WAVE_MODE(10)
            default: WAVE_MODE(0)
        }
    } else {
        switch (g_debug_mode) {
            FILL_MODE(1) FILL_MODE(2) FILL_MODE(3) FILL_MODE(4) FILL_MODE(5)
            default: FILL_MODE(0)
        }
    }
#else
    if (wave && b.n < HPK_WAVE_GUIDED_MIN)
        hipLaunchKernelGGL(WAVE_KERNEL_SMALL(0), grid, block, 0, c->stream, a);
    else if (wave)
        hipLaunchKernelGGL(WAVE_KERNEL(0), grid, block, 0, c->stream, a);
    else
        hipLaunchKernelGGL(DEC_KERNEL(0), grid, block, 0, c->stream, a);
#endif
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}
