// hpk_encode.hip — gfx950 batched canonical Huffman encode (RFC 7541 §5.2; the H-bit branch
// crates/loona-hpack/src/encoder.rs:299-307 never takes — the reference has no encoder).
//
// v2 (hpk_encode2): one 1024-thread workgroup per CU owns a contiguous literal range and encodes it
// in tiles of whole literals (<= 32 KiB of input, <= 2048 literals, output span <= the LDS image):
//   * every thread owns 32 consecutive input bytes of the tile (two 16-byte loads, in registers);
//   * a segmented scan of per-byte code lengths over the 1024 threads (literal starts reset it)
//     gives each byte its bit offset inside its literal;
//   * each byte's code is OR-ed into an LDS image of the tile's output span (big-endian dwords,
//     ds_or_b32, one or two per code), clipped at the literal's capacity;
//   * one thread per literal then pads the last byte with EOS's most significant bits (ones) and
//     writes out_len / status; the image goes out with 16-byte stores (bytewise in the span's two
//     end chunks, which neighbouring tiles own).
// A literal too large for a tile is encoded by one lane straight to global memory (v1's loop).
// v1 (hpk_encode_kernel, one lane per literal) stays as the comparison build (HPK_ENCODE_V1=1).
// (The kernel itself is in hpk_encode_kernel.h; the packed form is launched from hpk_encode_packed.hip.)
#include "hpk_encode_kernel.h"

namespace {

#define ENC_BLOCK 256

#ifdef HPK_DIAG
__global__ __launch_bounds__(ENC_BLOCK) void hpk_encode_kernel(EncodeArgs a) {
    __shared__ uint32_t s_code[256];
    __shared__ uint8_t s_len[256];
    if (threadIdx.x < 256) {
        s_code[threadIdx.x] = a.codes[threadIdx.x];
        s_len[threadIdx.x] = (uint8_t)a.codes[257 + threadIdx.x];
    }
    __syncthreads();
    for (uint32_t i = blockIdx.x * ENC_BLOCK + threadIdx.x; i < a.n; i += gridDim.x * ENC_BLOCK)
        encode_serial(a, s_code, s_len, i);
}
#endif

#ifdef HPK_DIAG
static int g_encode_v1 = -1, g_encode_cfg = 0;
#endif

}  // namespace

#ifdef HPK_DIAG
unsigned long long* hpk_g_eprof = nullptr;  // (hpk_device.h)
#endif

int hpk_launch_encode(hpk_ctx* c, const hpk_batch& b) {
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
    a.void_all = nullptr;
    int cfg = 0;
#ifdef HPK_DIAG
    // diagnostic build only: v1 (one lane per literal, no offset checks) and geometry variants
    if (g_encode_v1 < 0) {
        const char* e = getenv("HPK_ENCODE_V1");
        g_encode_v1 = e && atoi(e) ? 1 : 0;
        const char* w = getenv("HPK_ENCODE_CFG");
        g_encode_cfg = w ? atoi(w) : 0;
    }
    cfg = g_encode_cfg;
    if (g_encode_v1) {
        uint64_t blocks = ((uint64_t)b.n + ENC_BLOCK - 1) / ENC_BLOCK;
        const uint64_t max_blocks = (uint64_t)c->num_cu * 8;
        if (blocks > max_blocks) blocks = max_blocks;
        if (blocks < 1) blocks = 1;
        hipLaunchKernelGGL(hpk_encode_kernel, dim3((uint32_t)blocks), dim3(ENC_BLOCK), 0, c->stream, a);
        HIP_TRY(hipGetLastError());
        return HPK_E_OK;
    }
#endif
    // per = workgroups per CU; fewer when the batch is small (>= ~64 literals per workgroup)
    const int per = cfg == 1 ? 1 : 2;
    uint64_t blocks = ((uint64_t)b.n + kProdPerWg - 1u) / kProdPerWg;
    // (the small-call mode's persistent workgroups hold sm_wgs CUs, hpk_persist.h: left out of the grid)
    const uint64_t cus = (uint64_t)c->num_cu - (c->sm_launched && c->sm_max ? (uint64_t)c->sm_wgs : 0u);
    if (blocks > cus * per) blocks = cus * per;
    if (blocks < 1) blocks = 1;
    const dim3 grid((uint32_t)blocks);
    switch (cfg) {
#ifdef HPK_DIAG
        case 1:  // one 1024-thread workgroup per CU, 32 KiB tiles
            hipLaunchKernelGGL((hpk_encode2<1024, 112 * 1024, 2048, 32>), grid, dim3(1024), 0, c->stream, a);
            break;
        case 9:  // the product geometry with per-phase cycle counters (hpk_debug_encode_prof)
            if (!hpk_g_eprof) HIP_TRY(hipMalloc(&hpk_g_eprof, 16 * sizeof(unsigned long long)));
            HIP_TRY(hipMemsetAsync(hpk_g_eprof, 0, 16 * sizeof(unsigned long long), c->stream));
            a.prof = hpk_g_eprof;
            hipLaunchKernelGGL((hpk_encode2<kProdEB, kProdEO, kProdEQ, kProdEBytes, 1>), grid, dim3(kProdEB), 0,
                               c->stream, a);
            break;
#endif
        default:  // product: two 512-thread workgroups per CU, 32 bytes per thread
            hipLaunchKernelGGL((hpk_encode2<kProdEB, kProdEO, kProdEQ, kProdEBytes>), grid, dim3(kProdEB), 0,
                               c->stream, a);
    }
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}

extern "C" int hpk_test_encode_geometry(uint32_t* tile_bytes, uint32_t* image_bytes, uint32_t* tile_literals,
                                        uint32_t* thread_bytes, uint32_t* one_wg_literals) {
    if (!tile_bytes || !image_bytes || !tile_literals || !thread_bytes || !one_wg_literals) return HPK_E_INVAL;
    *tile_bytes = kProdEB * kProdEBytes;
    *image_bytes = kProdEO;
    *tile_literals = kProdEQ;
    *thread_bytes = kProdEBytes;
    *one_wg_literals = kProdPerWg;
    return HPK_E_OK;
}

#ifdef HPK_DIAG
// diagnostic build: the phase cycles of the last HPK_ENCODE_CFG=9 launch (16 x u64)
extern "C" int hpk_debug_encode_prof(unsigned long long* host16) {
    if (!hpk_g_eprof) return -1;
    return hipMemcpy(host16, hpk_g_eprof, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
