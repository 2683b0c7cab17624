// hpk_blkscan.hip — the header-block scan's own kernels (hpk_scan_blocks): the table-free half of
// Decoder::decode_with_cb (crates/loona-hpack/src/decoder.rs:368-450) on many blocks at once. A translation unit
// of its own. The call's steps (hpk_calls_blocks.hip strings them together):
//   * hpk_blkcount below, one lane per block (per-lane code in hpk_blkscan.h): the block's field count, its
//     listed-string count and its status (HPK_OK, or HPK_BAD_OFFSETS with the sticky flag and both counts 0);
//   * hpk_len_scan (hpk_pack.hip, as it is) over each count array: field_off and str_blk_off;
//   * hpk_blkemit below, one lane per block again: the same walk with a visitor that stores every field record
//     (one 16-byte store) at fields[field_off[b] ..) and every string window at str_off / str_end from
//     str_blk_off[b], each only below the caller's capacity.
// The lanes read the blocks with byte loads (hpk_strparse.h's reasoning: a block's lines come in once either
// way). One lane walks one whole block: a block of many thousands of small fields costs two dependent loads per
// field on that lane while its 255 neighbours wait (include/hpk.h states it).
#include "hpk_device.h"
#include "hpk_blkscan.h"

namespace {

constexpr uint32_t kBlkWg = 256;  // blocks per workgroup, one per lane (hpk_test_blkscan_geometry)

struct BlkArgs {
    const uint8_t* blob;
    uint32_t cap;
    const uint32_t* block_off;
    uint32_t nblocks;
    // the count pass's outputs
    uint32_t* nfields;
    uint32_t* nstrs;
    uint8_t* status;
    uint32_t* err;
    // the emit pass's inputs and outputs
    const uint32_t* field_off;
    const uint32_t* str_blk_off;
    uint4* fields;
    uint32_t fields_cap;
    uint32_t* str_off;
    uint32_t* str_end;
    uint32_t strs_cap;
};

__global__ __launch_bounds__(kBlkWg) void hpk_blkcount(BlkArgs a) {
    const uint32_t b = blockIdx.x * kBlkWg + threadIdx.x;
    if (b >= a.nblocks) return;
    const uint32_t lo = a.block_off[b], hi = a.block_off[b + 1];
    hpkblk::Counts n = {0u, 0u};
    uint32_t st = HPK_OK;
    if (lo > hi || hi > a.cap) {
        st = HPK_BAD_OFFSETS;
        *a.err = 1u;
    } else {
        hpkblk::NoVisit v;
        n = hpkblk::walk_block(a.blob, lo, hi, v);
    }
    a.nfields[b] = n.fields;
    a.nstrs[b] = n.strs;
    a.status[b] = (uint8_t)st;
}

struct EmitVisit {
    uint4* fields;
    uint32_t fbase, fields_cap;
    uint32_t* str_off;
    uint32_t* str_end;
    uint32_t sbase, strs_cap;
    // (bases and counts are sums of at most cap <= HPK_MAX_OFFSET one-octet items: no wrap)
    __device__ __forceinline__ void field(uint32_t i, const hpk_field& f) {
        const uint32_t j = fbase + i;
        if (j < fields_cap)
            fields[j] = make_uint4(f.index, sbase + f.str,
                                   (uint32_t)f.kind | (uint32_t)f.nstr << 8 | (uint32_t)f.err << 16 | (uint32_t)f.err_stage << 24,
                                   f.at);
    }
    __device__ __forceinline__ void string(uint32_t s, uint32_t off, uint32_t end) {
        const uint32_t j = sbase + s;
        if (j < strs_cap) {
            str_off[j] = off;
            str_end[j] = end;
        }
    }
};

__global__ __launch_bounds__(kBlkWg) void hpk_blkemit(BlkArgs a) {
    const uint32_t b = blockIdx.x * kBlkWg + threadIdx.x;
    if (b >= a.nblocks) return;
    const uint32_t lo = a.block_off[b], hi = a.block_off[b + 1];
    if (lo > hi || hi > a.cap) return;  // void: the count pass has said so
    EmitVisit v{a.fields, a.field_off[b], a.fields_cap, a.str_off, a.str_end, a.str_blk_off[b], a.strs_cap};
    (void)hpkblk::walk_block(a.blob, lo, hi, v);
}
}  // namespace

static_assert(sizeof(hpk_field) == 16, "hpk_field is one 16-byte store");

int hpk_launch_blkcount(hpk_ctx* c, const uint8_t* blob, uint32_t cap, const uint32_t* block_off, uint32_t nblocks,
                        uint32_t* nfields, uint32_t* nstrs, uint8_t* status) {
    BlkArgs a{};
    a.blob = blob;
    a.cap = cap;
    a.block_off = block_off;
    a.nblocks = nblocks;
    a.nfields = nfields;
    a.nstrs = nstrs;
    a.status = status;
    a.err = c->d_err;
    hipLaunchKernelGGL(hpk_blkcount, dim3((nblocks + kBlkWg - 1u) / kBlkWg), dim3(kBlkWg), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}

int hpk_launch_blkemit(hpk_ctx* c, const uint8_t* blob, uint32_t cap, const uint32_t* block_off, uint32_t nblocks,
                       const uint32_t* field_off, const uint32_t* str_blk_off, hpk_field* fields, uint32_t fields_cap,
                       uint32_t* str_off, uint32_t* str_end, uint32_t strs_cap) {
    BlkArgs a{};
    a.blob = blob;
    a.cap = cap;
    a.block_off = block_off;
    a.nblocks = nblocks;
    a.field_off = field_off;
    a.str_blk_off = str_blk_off;
    a.fields = reinterpret_cast<uint4*>(fields);
    a.fields_cap = fields_cap;
    a.str_off = str_off;
    a.str_end = str_end;
    a.strs_cap = strs_cap;
    hipLaunchKernelGGL(hpk_blkemit, dim3((nblocks + kBlkWg - 1u) / kBlkWg), dim3(kBlkWg), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}

extern "C" int hpk_test_blkscan_geometry(uint32_t* wg_blocks) {
    if (!wg_blocks) return HPK_E_INVAL;
    *wg_blocks = kBlkWg;
    return HPK_E_OK;
}
