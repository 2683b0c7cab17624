// hpk_device.h — shared between the device translation units of libhpk (context, decode, encode, pack).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/hpk.h"
#include "hpk_chunks.h"
#include "hpk_code.h"
#include "hpk_internal.h"

// A blob pointer as the kernels take it: the 16-byte-aligned address at or below it and the bytes between.
template <class T>
struct hpk_split16 {
    T* base;
    uint32_t mis;
};
template <class T>
inline hpk_split16<T> split16(T* p) {
    const uintptr_t u = (uintptr_t)p;
    return {(T*)(u & ~(uintptr_t)15), (uint32_t)(u & 15)};
}

// A grow-only device buffer.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;  // bytes
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

// The scratch of the device-pointer calls on one stream. Calls on different streams may overlap, so each
// stream that uses the context gets a slot of its own (two calls on two streams never share a list, a
// layout or the cursor: ADVICE r4); a stream's calls are ordered, so its slot is reused without a wait.
// A call takes its stream's slot (hpk_slot_acquire), sizes the buffers it uses (hpk_slot_reserve), launches, and
// marks the slot used after its last operation on the stream (hpk_slot_commit), all in hpk_ctx.hip. The rules:
//   * While only the context's own stream has used it, no event is created or recorded (an event record
//     per launch cost about 1 us of a ~23 us small call).
//   * The first use by a second stream switches to events. It synchronises the own stream once, and clears
//     the event-set flag only of slots last used on the own stream: a slot used on another stream keeps
//     its recorded event, which the own-stream wait does not cover.
//   * A launch on a stream that the context does not own always records its slot's event.
//   * A slot is waited for through its event, or through the own stream if it has none (by the rule above
//     it was then last used there). It is never waited for through another stream's handle: the caller
//     may have destroyed that stream.
//   * With all slots taken, the oldest is reused round-robin once its event has completed.
//   * A buffer is freed or regrown only after the slot is drained, and a call drains at most once.
//   * hpk_ctx_destroy waits on the set events before it frees.
struct hpk_slot {
    hipStream_t stream = nullptr;  // the stream that holds it, if `used` (nullptr is also the legacy stream)
    bool used = false;             // a call has reserved it: launches that read its buffers may be in flight
    hipEvent_t ev = nullptr;       // created at the slot's first use once the context records events
    bool ev_set = false;           // ev was recorded after the slot's last launch
    DevBuf long_list;     // the decode kernels' long-literal list: one u32 per literal of the batch
    // the workgroup-fill kernel's compacted form: the bound layout, the bound scan's scratch, the output cursor
    DevBuf cp_bound, cp_tmp, cp_cursor;
    // the packed form: the region decode's scratch blob and its bound layout, and the two scans' scratch (the
    // pack alone uses only the last)
    DevBuf pk_scratch, pk_bound, pk_tmp;
    // the string-literal encode's host form: the staged input, arrays and output (hpk_encode_strings_packed)
    DevBuf str_stage;
    // the string-literal decode (hpk_decode_strings_packed): the parse step's per-string arrays and the gather's
    // offsets, the gathered Huffman blob, and the host form's staged input, arrays and output
    DevBuf sd_meta, sd_hblob, sd_stage;
    // the header-block scan (hpk_scan_blocks): the count pass's two arrays; the staged input and arrays of its host
    // form and of the block decoder's device-scan path; and that path's outputs, sized once the totals are known
    DevBuf bs_meta, bs_stage, bs_out;
    // the block decoder's device-apply path: the lists, the tables, the results and the header records
    DevBuf ba_buf;
    // the header-block plan (hpk_plan_blocks): the two hashes per header
    DevBuf bp_hash;
    // the block encoder's device-plan path: the arena, the lists, the tables, the items and the coded bytes
    DevBuf bp_buf;
    // the frame scan (hpk_scan_frames): the count pass's three arrays; the staged input, states and arrays of its host
    // form and of hpk_h2_read_frames' device path; and that path's lists and gathered blocks, sized once the totals
    // are known (hpk_frame_blocks keeps its nfrags + 1 packed offsets there)
    DevBuf fs_meta, fs_stage, fs_out;
    // the frame write's host form (hpk_write_frames): the staged blocks, arrays and wire octets
    DevBuf fw_stage;
    // every buffer above: the one list of them (hpk_ctx_destroy frees through it)
    static constexpr size_t kBufs = 21;
    template <class F>
    void each_buf(F f) {
        for (DevBuf* b : {&long_list, &cp_bound, &cp_tmp, &cp_cursor, &pk_scratch, &pk_bound, &pk_tmp, &str_stage, &sd_meta, &sd_hblob,
                          &sd_stage, &bs_meta, &bs_stage, &bs_out, &ba_buf, &bp_hash, &bp_buf, &fs_meta, &fs_stage, &fs_out, &fw_stage})
            f(*b);
    }
};
// (the buffers are the slot's last members: one added and not listed in each_buf fails here)
static_assert(sizeof(hpk_slot) == offsetof(hpk_slot, long_list) + hpk_slot::kBufs * sizeof(DevBuf), "hpk_slot::each_buf");

struct hpk_ctx {
    int device = 0;
    int num_cu = 256;
    int decode_kernel = HPK_DECODE_AUTO;  // hpk_ctx_set_decode_kernel
    int block_scan = HPK_BLOCK_SCAN_HOST;  // hpk_ctx_set_block_scan
    int block_apply = HPK_BLOCK_APPLY_HOST;  // hpk_ctx_set_block_apply
    int block_plan = HPK_BLOCK_PLAN_HOST;  // hpk_ctx_set_block_plan
    int frame_scan = HPK_FRAME_SCAN_HOST;  // hpk_ctx_set_frame_scan
    int frame_write = HPK_FRAME_WRITE_HOST;  // hpk_ctx_set_frame_write
    uint64_t frame_write_calls = 0;  // hpk_h2_write_headers calls the device framing answered (hpk_test_frame_write_calls)
    uint64_t plan_calls = 0;  // hpk_henc_encode_blocks calls the device-plan path answered (hpk_test_plan_calls)
    hpk_header* d_static = nullptr;  // hpk_static_table's 61 records, uploaded by the first hpk_apply_blocks
    hipStream_t own = nullptr;
    hipStream_t stream = nullptr;
    uint32_t* d_lut2 = nullptr;
    uint32_t* d_lut3 = nullptr;
    uint32_t* d_lut13 = nullptr;
    uint16_t* d_lo = nullptr;
    uint32_t* d_codes = nullptr;  // [0,257) code, [257,514) length
    // grow-only scratch for HPK_PTR_HOST calls
    uint8_t* d_in = nullptr;
    size_t d_in_cap = 0;
    uint8_t* d_out = nullptr;
    size_t d_out_cap = 0;
    uint32_t* d_meta = nullptr;  // in_off | out_off | out_len
    size_t d_meta_cap = 0;
    uint8_t* d_st = nullptr;
    size_t d_st_cap = 0;
    // page-locked host staging for the block-level calls (hpk_ctx_pinned), grow-only
    void* h_pin = nullptr;
    size_t h_pin_cap = 0;
    // host-pointer pipeline: copy-in and copy-out streams + per-chunk events (created lazily)
    static constexpr int kMaxChunks = kHpkMaxChunks;  // (hpk_chunks.h)
    hipStream_t h2d = nullptr;
    hipStream_t d2h = nullptr;
    hipEvent_t ev_in[kMaxChunks] = {};
    hipEvent_t ev_run[kMaxChunks] = {};
    hipEvent_t ev_out[kMaxChunks] = {};  // chunk j's results are in host memory
    // sticky error flag: host-mapped, written (plain store of 1) by a kernel that saw bad offsets
    uint32_t* h_err = nullptr;
    uint32_t* d_err = nullptr;
    // the per-stream slots (hpk_slot above)
    static constexpr int kSlots = 8;
    hpk_slot slots[kSlots];
    int slot_next = 0;        // the round-robin victim when all are taken
    bool slot_events = false;  // more than one stream has used the context: slots carry events
    // the small-call mode (hpk_ctx_set_small_mode, hpk_persist.h): a persistent kernel of sm_wgs
    // workgroups on its own stream takes synchronous device-pointer batches of <= sm_max literals
    uint32_t sm_max = 0;
    int sm_wgs = 0;
    uint32_t sm_idle_ms = 0;
    hipStream_t sm_stream = nullptr;
    void* h_sm = nullptr;           // hpkdec::PersistCtl, coherent host memory
    void* d_sm = nullptr;           // its device-visible address
    uint32_t* d_sm_dev = nullptr;   // [0] workgroups finished, [1] command broadcast, [2] declined request
    uint32_t sm_req = 0;            // the last request issued
    bool sm_launched = false;       // a kernel was launched on sm_stream (it may have exited since)
    uint64_t sm_calls = 0;          // calls it answered (hpk_test_small_calls)
};

// The small-call mode (hpk_decode.hip): hpk_persist_call decodes a synchronous device-pointer batch through
// the persistent kernel if the mode is on, the batch small enough and the caller's stream idle (*handled);
// hpk_persist_stop ends the kernel and waits for it.
int hpk_persist_call(hpk_ctx* c, const struct hpk_batch& b, bool* handled);
int hpk_persist_start(hpk_ctx* c);
int hpk_persist_stop(hpk_ctx* c);

// One batch call as the launchers see it: capacities clamped to HPK_MAX_OFFSET (offsets above
// them are bad whatever the buffer size).
struct hpk_batch {
    const uint8_t* in_blob;
    uint32_t in_cap;
    const uint32_t* in_off;
    uint32_t n;
    uint8_t* out_blob;
    uint32_t out_cap;
    const uint32_t* out_off;
    uint32_t* out_len;
    uint8_t* status;
};

int hpk_set_err(const char* what, hipError_t e);
int hpk_set_err_msg(const char* what, int code);

#define HIP_TRY(call)                                            \
    do {                                                         \
        hipError_t _e = (call);                                  \
        if (_e != hipSuccess) return hpk_set_err(#call, _e);     \
    } while (0)

// The launchers enqueue on the ctx stream. long_list: the long-literal list of the caller's slot, b.n
// entries (the caller acquired and reserved the slot, and commits it after its last operation).
int hpk_launch_decode(hpk_ctx* c, const hpk_batch& b, uint32_t* long_list);
// The compacted mode, co_off the caller's output offsets. wave (hpk_compact_wave): the wave-fill kernel,
// which makes its bound layout from in_off itself and writes co_off[n]; otherwise the workgroup-fill
// kernel, b.out_off the bound layout made by hpk_bound_scan and cursor the (zeroed) output cursor.
bool hpk_compact_wave(const hpk_ctx* c, uint32_t n);
int hpk_launch_decode_compact(hpk_ctx* c, const hpk_batch& b, uint32_t* co_off, uint32_t* long_list, uint32_t* cursor,
                              bool wave);
int hpk_launch_encode(hpk_ctx* c, const hpk_batch& b);
#ifdef HPK_DIAG
// diagnostic build: hpk_encode2's phase cycles of the last HPK_ENCODE_CFG=9 launch, either form's (16 x u64 of
// device memory, allocated at the first such launch; defined in hpk_encode.hip)
extern unsigned long long* hpk_g_eprof;
#endif
// The packed encode's three steps (hpk_encode_batch_packed), on the ctx stream. The length pass: out_len[i] =
// literal i's encoded bytes, 0 with bad offsets (sticky error flag; status, if not null, HPK_OK or
// HPK_BAD_OFFSETS). The length scan (hpk_pack.hip): out_off (n + 1 entries) = the exclusive sum of len, all 0
// when the total passes HPK_MAX_OFFSET (flag set); tmp: hpk_pack_tmp_bytes(n) bytes of device scratch, and
// hpk_len_scan_verdict(tmp, n) the word in it that is then nonzero. The encode into b.out_off's exact regions,
// clipped at b.out_cap, void_all that word.
int hpk_launch_enclen(hpk_ctx* c, const uint8_t* in_blob, uint32_t in_cap, const uint32_t* in_off, uint32_t n,
                      uint32_t* out_len, uint8_t* status);
int hpk_len_scan(hpk_ctx* c, const uint32_t* len, uint32_t n, uint32_t* out_off, void* tmp);
const unsigned long long* hpk_len_scan_verdict(const void* tmp, uint32_t n);
int hpk_launch_encode_packed(hpk_ctx* c, const hpk_batch& b, const unsigned long long* void_all);
// The string-literal encode's own steps (hpk_encode_strings.hip), on the ctx stream, around hpk_launch_enclen and
// hpk_len_scan. The form step: out_len[i], literal i's Huffman bytes as hpk_launch_enclen left them, becomes the
// length of its representation under policy[i] (null: all HPK_STR_AUTO), 0 with bad offsets or a policy above 3
// (sticky error flag; status, if not null, HPK_OK or HPK_BAD_OFFSETS). The emit into b.out_off's exact regions,
// clipped at b.out_cap, void_all the length scan's verdict.
int hpk_launch_strlen_form(hpk_ctx* c, uint32_t in_cap, const uint32_t* in_off, uint32_t n, const uint8_t* policy,
                           uint32_t* out_len, uint8_t* status);
int hpk_launch_encode_strings(hpk_ctx* c, const hpk_batch& b, const uint8_t* policy, const unsigned long long* void_all);
// The bound layout (hpk_pack.hip): out[i] = sum over j < i of the 4-rounded decoded bound of literal j, mod
// 2^32 (n + 1 entries); tmp: hpk_bound_tmp_bytes(n) bytes of device scratch.
size_t hpk_bound_tmp_bytes(uint32_t n);
int hpk_bound_scan(hpk_ctx* c, const uint32_t* in_off, uint32_t n, uint32_t* out, void* tmp);
// The ordered pack (hpk_pack.hip), on the ctx stream: dst_off (n + 1 entries) = the exclusive sum of the n
// lengths, a literal with src_off + src_len > src_cap counting 0 (sticky error flag), then literal i's bytes
// src_blob[src_off[i] ..) to dst_blob[dst_off[i] ..), of which only those below dst_cap are written. tmp:
// hpk_pack_tmp_bytes(n) bytes of device scratch; total_bound: an upper bound of dst_off[n] (it sizes the grid).
size_t hpk_pack_tmp_bytes(uint32_t n);
int hpk_pack_launch(hpk_ctx* c, const uint8_t* src_blob, uint32_t src_cap, const uint32_t* src_off, const uint32_t* src_len,
                    uint32_t n, uint8_t* dst_blob, uint32_t dst_cap, uint32_t* dst_off, void* tmp, uint64_t total_bound);

// The string-literal decode's own steps (hpk_decode_strings.hip), on the ctx stream, around hpk_pack_launch,
// hpk_bound_scan, hpk_launch_decode and hpk_len_scan. The parse: string i's window in_blob[str_off[i] .. str_end[i])
// gives pst[i] (HPK_OK, HPK_BAD_OFFSETS with the sticky flag, or one of the three prefix and length errors),
// start[i] (the payload's first byte), hlen[i] / rlen[i] (a Huffman / a raw payload's bytes, the other 0; both 0
// unless pst is HPK_OK) and consumed[i] (if not null). The merge: out_len / status hold the region decode of the
// gathered Huffman payloads (offsets hoff, regions bound, of region_cap bytes) and become the final ones; src
// (in: start) becomes the offset of string i's bytes in the source sel[i] names (0 the region scratch, 1 the input
// blob). The two-source pack: hpk_pack_launch's kernel with that choice per literal, dst_off given (n + 1).
int hpk_launch_strparse(hpk_ctx* c, const uint8_t* in_blob, uint32_t in_cap, const uint32_t* str_off, const uint32_t* str_end,
                        uint32_t n, uint32_t* start, uint32_t* hlen, uint32_t* rlen, uint8_t* pst, uint32_t* consumed);
int hpk_launch_strmerge(hpk_ctx* c, uint32_t n, uint32_t* src, const uint32_t* hlen, const uint32_t* rlen, const uint8_t* pst,
                        const uint32_t* hoff, const uint32_t* bound, uint32_t region_cap, uint32_t* out_len, uint8_t* status,
                        uint8_t* sel);
int hpk_pack2_launch(hpk_ctx* c, const uint8_t* src0, uint32_t cap0, const uint8_t* src1, uint32_t cap1, const uint32_t* src_off,
                     const uint8_t* sel, uint32_t n, uint8_t* dst_blob, uint32_t dst_cap, const uint32_t* dst_off,
                     uint64_t total_bound);

// The header-block scan's two passes (hpk_blkscan.hip), on the ctx stream, around hpk_len_scan. The count pass:
// block b = blob[block_off[b] .. block_off[b+1]) gives nfields[b], nstrs[b] and status[b] (HPK_OK, or
// HPK_BAD_OFFSETS with the sticky flag and both counts 0). The emit pass: the same walk, block b's records to
// fields[field_off[b] ..) and its string windows to str_off / str_end from str_blk_off[b], each only below its
// capacity; fields is 16-byte aligned.
int hpk_launch_blkcount(hpk_ctx* c, const uint8_t* blob, uint32_t cap, const uint32_t* block_off, uint32_t nblocks,
                        uint32_t* nfields, uint32_t* nstrs, uint8_t* status);
int hpk_launch_blkemit(hpk_ctx* c, const uint8_t* blob, uint32_t cap, const uint32_t* block_off, uint32_t nblocks,
                       const uint32_t* field_off, const uint32_t* str_blk_off, hpk_field* fields, uint32_t fields_cap,
                       uint32_t* str_off, uint32_t* str_end, uint32_t strs_cap);

// The header-block apply's kernel (hpk_blkapply.hip), on the ctx stream: hpk_apply_blocks' arguments as they are
// (headers_cap clamped to 32 bits, as field_off's entries are) and the static records in device memory. results is
// zeroed by the caller; fields, headers and tab_ent are 16-byte aligned.
int hpk_launch_blkapply(hpk_ctx* c, const hpk_field* fields, const uint32_t* field_off, uint32_t nblocks, const uint32_t* out_off,
                        const uint32_t* out_len, const uint8_t* status, uint32_t nstrs, uint32_t str_base, uint32_t static_base,
                        const uint32_t* dec_blk_off, const uint32_t* dec_blk, uint32_t ndecs, hpk_dtab* tabs, hpk_header* tab_ent,
                        uint64_t tab_ent_cap, hpk_header* headers, uint32_t headers_cap, hpk_block_result* results,
                        const hpk_header* d_static);

// The header-block plan's two kernels (hpk_blkplan.hip), on the ctx stream: hpk_plan_blocks' arguments as they are
// (the capacities clamped to 32 bits), hashes 8 bytes of device scratch per header, and the static records in device
// memory. The default-and-hash pass runs when hdrs_cap > 0, the plan kernel when there are encoders and blocks. reps
// and tab_ent are 16-byte aligned, arena + prefix_base 4-byte aligned.
int hpk_launch_blkplan(hpk_ctx* c, uint8_t* arena, uint32_t arena_cap, uint32_t static_base, uint32_t fields_base,
                       uint32_t prefix_base, const uint32_t* field_off, const uint32_t* hdr_off, uint32_t nblocks, uint32_t hdrs_cap,
                       const uint32_t* enc_blk_off, const uint32_t* enc_blk, const uint8_t* enc_flags, uint32_t nencs, hpk_dtab* tabs,
                       hpk_header* tab_ent, uint64_t tab_ent_cap, hpk_hrep* reps, uint32_t* item_off, uint32_t* item_len,
                       uint8_t* item_policy, void* hashes, const hpk_header* d_static);

// boff[b] = out_off[3 * hdr_off[b]] for b <= nblocks: where block b's bytes begin in the strings call's output.
int hpk_launch_blkplan_boff(hpk_ctx* c, const uint32_t* out_off, const uint32_t* hdr_off, uint32_t nblocks, uint32_t* boff);

// The frame scan's passes (hpk_frmscan.hip), on the ctx stream, around hpk_len_scan and hpk_pack_launch. The count pass:
// connection c = blob[off[c] .. off[c+1]) with state conns[c] gives nblk[c], nclosed[c] and nopen[c], all 0 with the
// sticky flag for a void connection; it does not write the states. The emit pass: the same walk, the block records to
// blocks from conn_blk_off[c], the closed windows to frag_off / frag_len from conn_frag_off[c], the open ones to
// open_off / open_len from conn_open_off[c], each only below its capacity, then the state; conns and blocks are
// 16-byte aligned. hpk_launch_frmboff: block_off[b] = dst_off[blocks[b].frag] (clamped, hpk_frame_blocks) for b <
// nblocks and block_off[nblocks] = dst_off[nfrags].
int hpk_launch_frmcount(hpk_ctx* c, const uint8_t* blob, uint32_t cap, const uint32_t* off, uint32_t nconn, const hpk_fconn* conns,
                        uint32_t* nblk, uint32_t* nclosed, uint32_t* nopen);
int hpk_launch_frmemit(hpk_ctx* c, const uint8_t* blob, uint32_t cap, const uint32_t* off, uint32_t nconn, hpk_fconn* conns,
                       const uint32_t* conn_blk_off, const uint32_t* conn_frag_off, const uint32_t* conn_open_off, hpk_fblock* blocks,
                       uint32_t blocks_cap, uint32_t* frag_off, uint32_t* frag_len, uint32_t frags_cap, uint32_t* open_off,
                       uint32_t* open_len, uint32_t opens_cap);
int hpk_launch_frmboff(hpk_ctx* c, const uint32_t* dst_off, uint32_t nfrags, const hpk_fblock* blocks, uint32_t nblocks,
                       uint32_t* block_off);

// The frame write's steps (hpk_frmwrite.hip), on the ctx stream: wire_off (nblocks + 1 entries) = the exclusive sum of
// the blocks' wire lengths, a void block counting 0 (sticky flag), all 0 when the total passes HPK_MAX_OFFSET; status
// HPK_OK or HPK_BAD_OFFSETS; then block b's frames to out_blob[wire_off[b] ..), of which only the octets below out_cap
// are written. tmp: hpk_pack_tmp_bytes(nblocks) bytes of device scratch.
int hpk_frmwrite_launch(hpk_ctx* c, const uint8_t* blocks, uint32_t cap, const uint32_t* block_off, uint32_t nblocks,
                        const uint32_t* stream_id, const uint32_t* max_frame, uint8_t* out_blob, uint32_t out_cap,
                        uint32_t* wire_off, uint8_t* status, void* tmp);

__device__ __forceinline__ uint32_t hpk_bswap32(uint32_t x) { return __builtin_bswap32(x); }
