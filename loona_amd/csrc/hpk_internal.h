// hpk_internal.h — declarations shared between the host (hpk_cpu.cpp) and device (hpk_gpu.hip)
// halves of libhpk. Not part of the C ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/hpk.h"
#include "hpk_code.h"

const hpk_tables* hpk_get_tables();
int hpk_cpu_decode(const hpk_tables* t, const uint8_t* in, size_t n, uint8_t* out, size_t cap,
                   size_t* out_len);
int hpk_cpu_encode(const hpk_tables* t, const uint8_t* in, size_t n, uint8_t* out, size_t cap,
                   size_t* out_len);

// The block decoder's device-scan path (hpk_ctx.hip: hpk_blocks_device; used by hpk_hpack.cpp): what it leaves
// in the context's page-locked area, valid until the context's next block call.
struct hpk_blkdev {
    const hpk_field* fields;
    const uint32_t* field_off;  // nblocks + 1
    const uint32_t* out_off;    // nstrs + 1: string s is arena[out_off[s] .. out_off[s] + out_len[s])
    const uint32_t* out_len;
    const uint8_t* status;  // hpk_status per string
    const uint8_t* arena;
    uint32_t nfields, nstrs;
    long us_scan, us_strings, us_back;  // wall times: upload, count, scans, totals / emit, string decode, arrays / bytes
};
int hpk_blocks_device(hpk_ctx* c, const uint8_t* blocks, const uint32_t* block_off, uint32_t nblocks, hpk_blkdev* o);
int hpk_ctx_block_scan(const hpk_ctx* c);  // hpk_ctx_set_block_scan's value (HPK_BLOCK_SCAN_HOST for no context)
