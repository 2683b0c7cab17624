// hpk_internal.h — declarations shared between the host units of libhpk (hpk_cpu.cpp, hpk_hdec.cpp, hpk_henc.cpp, hpk_h2.cpp) and its
// device half (hpk_ctx.hip and the hpk_calls_*.hip call layer). Not part of the C ABI.
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

// hpk_ctx.hip: the context's page-locked host staging area, grown to at least `bytes` (grow-only)
int hpk_ctx_pinned(hpk_ctx* ctx, size_t bytes, void** p);
// hpk_calls_batch.hip: a trusted host batch whose chunks can be waited for one by one (the block decoder's form)
int hpk_decode_host_begin(hpk_ctx* c, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off, uint32_t n,
                          uint8_t* out_blob, size_t out_cap, const uint32_t* out_off, uint32_t* out_len,
                          uint8_t* status, int* nchunks, uint32_t* cut);
int hpk_host_chunk_wait(hpk_ctx* c, int j);
int hpk_decode_host_end(hpk_ctx* c);
int hpk_ctx_max_chunks();

// The block decoder's device-scan path (hpk_calls_blocks.hip: hpk_blocks_device; used by hpk_hdec.cpp): what it leaves
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
// With a plan (HPK_BLOCK_APPLY_DEVICE), hpk_apply_blocks' kernel runs behind those steps. The arena it refers to is
// the host's to build: the static text at 0, the tables' prior bytes behind it, the packed strings at str_base; no
// byte of it goes to the device, which moves references only. applied says which set of outputs is back.
struct hpk_applyplan {
    // in (host memory): every block in exactly one decoder's list, the tables as hpk_apply_blocks takes them
    const uint32_t* dec_blk_off;
    const uint32_t* dec_blk;
    uint32_t ndecs;
    const hpk_dtab* tabs;
    const hpk_header* tab_ent;
    uint32_t nent;
    uint32_t str_base;
    // out (the page-locked area). applied == 1: no block was deferred; results (nblocks), tabs_out (ndecs), headers
    // (hpk_blkdev.nfields records, those no block covers zero), ent_out (nent) and, in hpk_blkdev.arena, packed_len
    // packed bytes; the rest of hpk_blkdev is not filled. applied == 0: hpk_blkdev as without a plan.
    int applied;
    const hpk_block_result* results;
    const hpk_dtab* tabs_out;
    const hpk_header* headers;
    const hpk_header* ent_out;
    uint32_t packed_len;
    long us_apply;  // wall time: the uploads, the kernel, results and tables back
};
int hpk_blocks_device(hpk_ctx* c, const uint8_t* blocks, const uint32_t* block_off, uint32_t nblocks, hpk_blkdev* o,
                      hpk_applyplan* plan = nullptr);

// The block encoder's device-plan path (hpk_calls_blocks.hip: hpk_plan_device; used by hpk_henc.cpp, HPK_BLOCK_PLAN_DEVICE):
// the host lays out hpk_plan_blocks' inputs, the device plans, gathers the items with the ordered pack and codes them
// with hpk_encode_strings_packed's steps. Everything is on the host when it returns HPK_E_OK.
struct hpk_planjob {
    // in (host memory): hpk_plan_blocks' arguments; the static text lies at 0 of the arena, of which the bytes below
    // prefix_base go up and the 4 * nh bytes of the prefix area are only reserved; hdr_off starts at 0
    const uint8_t* arena;
    uint32_t fields_base, prefix_base;
    const uint32_t* field_off;  // 2 nh + 1
    const uint32_t* hdr_off;    // nblocks + 1
    uint32_t nblocks, nh;
    const uint32_t* enc_blk_off;
    const uint32_t* enc_blk;
    const uint8_t* enc_flags;
    uint32_t nencs;
    // in / out (host memory): the tables, and their final entries
    hpk_dtab* tabs;
    hpk_header* tab_ent;
    uint32_t nent;
    // out: block b's bytes are bytes[block_off[b] .. block_off[b+1]); block_off the caller's (nblocks + 1), bytes
    // from malloc, the caller's to free (null when the call fails)
    uint32_t* block_off;
    uint8_t* bytes;
    long us_up, us_plan, us_items, us_strings, us_back;  // wall times of the passes (the stream is waited for only under HPK_HENC_TIMING)
};
int hpk_plan_device(hpk_ctx* c, hpk_planjob* job);
void hpk_ctx_plan_answered(hpk_ctx* c);    // the caller has committed such a call's tables (hpk_test_plan_calls counts it)
int hpk_ctx_block_plan(const hpk_ctx* c);  // hpk_ctx_set_block_plan's value (HPK_BLOCK_PLAN_HOST for no context)
int hpk_ctx_block_scan(const hpk_ctx* c);  // hpk_ctx_set_block_scan's value (HPK_BLOCK_SCAN_HOST for no context)
int hpk_ctx_block_apply(const hpk_ctx* c);  // hpk_ctx_set_block_apply's value (HPK_BLOCK_APPLY_HOST for no context)

// hpk_h2_read_frames' device frame scan (hpk_calls_frames.hip: hpk_frames_device; used by hpk_h2.cpp,
// HPK_FRAME_SCAN_DEVICE). hpk_h2.cpp reaches it through a pointer that it defines itself and hpk_ctx_create installs
// (hpk_h2_set_frames_device), so the host units take no symbol of the device half for it: the pointer is null where
// only the host half is linked. The installed function returns HPK_FRAMES_NOT_SELECTED for a context on
// HPK_FRAME_SCAN_HOST (a null job asks just that: HPK_E_OK says selected), and else HPK_E_OK with everything on the
// host, or a negative code with nothing written.
struct hpk_frmjob {
    // in (host memory): the call's bytes and offsets as hpk_h2_read_frames got them; the states as hpk_scan_frames
    // takes them, a pending connection's carry_off counted from off[nconn]: into `carry`, the held fragment bytes of
    // the pending connections end to end (ncarry bytes)
    const uint8_t* bytes;
    const uint32_t* off;
    uint32_t nconn;
    hpk_fconn* conns;  // in / out
    const uint8_t* carry;
    uint32_t ncarry;
    // out, the caller's arrays: conn_open_off (nconn + 1); the rest from malloc, the caller's to free (null when the
    // call fails): the block records, block_off (nblocks + 1), the blocks' bytes (block_off[nblocks] of them) and the
    // open windows (conn_open_off[nconn] of them; an offset at or past off[nconn] lies in `carry`)
    uint32_t* conn_open_off;
    uint32_t nblocks;
    hpk_fblock* blocks;
    uint32_t* block_off;
    uint8_t* blk;
    uint32_t* open_off;
    uint32_t* open_len;
};
enum { HPK_FRAMES_NOT_SELECTED = 1 };
typedef int (*hpk_frames_device_fn)(hpk_ctx* c, hpk_frmjob* job);
void hpk_h2_set_frames_device(hpk_frames_device_fn fn);  // hpk_h2.cpp
int hpk_frames_device(hpk_ctx* c, hpk_frmjob* job);      // hpk_calls_frames.hip
// The frame write's host arithmetic (hpk_h2.cpp, hpk_calls_frames.hip): a header block of L octets takes
// max(1, ceil(L / m)) frames of 9 octets more each for a frame size of m >= 1. The device states the same in
// hpk_frmwrite.h (fw_frames, fw_wire_len: __device__ code the host units cannot include);
// tests/test_frmwrite_emulation.py and tests/test_frames_write_cases.py hold both to the one Python model.
static inline uint64_t hpk_wire_len(uint32_t L, uint32_t m) {
    const uint64_t f = (uint64_t)(L / m) + (L % m != 0u ? 1u : 0u);
    return (uint64_t)L + 9u * (f ? f : 1u);
}
static inline bool hpk_max_frame_ok(uint32_t m) { return m >= 1u && m <= 0xFFFFFFu; }

// hpk_h2_write_headers' device framing (hpk_calls_frames.hip: hpk_write_device; used by hpk_h2.cpp,
// HPK_FRAME_WRITE_DEVICE), reached like the frame scan above through a pointer that hpk_h2.cpp defines and
// hpk_ctx_create installs (hpk_h2_set_write_device). The installed function takes hpk_write_frames' host-pointer
// arguments. It returns HPK_FRAMES_NOT_SELECTED for a context on HPK_FRAME_WRITE_HOST, and else HPK_E_OK with the
// octets and wire_off on the host (the context's count of answered calls raised), or a negative code: the caller
// then frames on the host.
typedef int (*hpk_write_device_fn)(hpk_ctx* c, const uint8_t* blocks, size_t cap, const uint32_t* block_off, uint32_t nblocks,
                                   const uint32_t* stream_id, const uint32_t* max_frame, uint8_t* out_blob, size_t out_cap,
                                   uint32_t* wire_off, uint8_t* status);
void hpk_h2_set_write_device(hpk_write_device_fn fn);  // hpk_h2.cpp
int hpk_write_device(hpk_ctx* c, const uint8_t* blocks, size_t cap, const uint32_t* block_off, uint32_t nblocks,
                     const uint32_t* stream_id, const uint32_t* max_frame, uint8_t* out_blob, size_t out_cap, uint32_t* wire_off,
                     uint8_t* status);  // hpk_calls_frames.hip
// hpk_henc.cpp: hpk_test_fail_batches' count, taken by one: 0, or the injected failure's code with its message set
int hpk_test_take_failure();
