// hpk_calls_blocks.hip — the header-block entry points of the C ABI (include/hpk.h): scan, apply and plan, and the
// block codec's device paths (hpk_hdec.cpp and hpk_henc.cpp call them).
#include <stdlib.h>

#include <chrono>

#include "hpk_calls.h"

// Wall time in microseconds since it was made or last lapped.
struct stopwatch {
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    long us() const { return (long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t).count(); }
    long lap() {
        const auto t0 = t;
        t = std::chrono::steady_clock::now();
        return (long)std::chrono::duration_cast<std::chrono::microseconds>(t - t0).count();
    }
};

// The header-block scan's steps on device arrays (hpk_blkscan.hip has the list), s the stream's slot with
// bs_meta (8 bytes per block) and pk_tmp (hpk_pack_tmp_bytes(nblocks)) reserved: the count pass and the two scans.
// The emit pass is the caller's (the block decoder sizes its outputs by the totals before it emits).
static int blkscan_counts(hpk_ctx* c, hpk_slot* s, const uint8_t* blocks, uint32_t cap, const uint32_t* block_off,
                          uint32_t nblocks, uint32_t* field_off, uint32_t* str_blk_off, uint8_t* status) {
    uint32_t* nf = s->bs_meta.as<uint32_t>();
    uint32_t* ns = nf + nblocks;
    int rc;
    if ((rc = hpk_launch_blkcount(c, blocks, cap, block_off, nblocks, nf, ns, status)) ||
        (rc = hpk_len_scan(c, nf, nblocks, field_off, s->pk_tmp.p)))
        return rc;
    return hpk_len_scan(c, ns, nblocks, str_blk_off, s->pk_tmp.p);
}

// The end of a scan call: a synchronous one reads both totals back with the wait, then reports bad offsets
// (HPK_E_INVAL) before a list that did not fit (HPK_E_NOSPACE).
static int blkscan_end(hpk_ctx* c, const uint32_t* field_off_n, size_t fields_cap, const uint32_t* str_blk_off_n,
                       size_t strs_cap, int flags) {
    if (flags & HPK_ASYNC) return HPK_E_OK;
    uint32_t tot[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&tot[0], field_off_n, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&tot[1], str_blk_off_n, 4, hipMemcpyDeviceToHost, c->stream));
    if (int rc = hpk_call_end(c, flags)) return rc;
    if ((size_t)tot[0] > fields_cap) return hpk_set_err_msg("the field records pass fields_cap", HPK_E_NOSPACE);
    if ((size_t)tot[1] > strs_cap) return hpk_set_err_msg("the string windows pass strs_cap", HPK_E_NOSPACE);
    return HPK_E_OK;
}

// The host form: offsets checked before anything is copied, the blocks staged in one piece (at their own
// offsets) into the slot's scratch beside the arrays, the steps, the totals read back, then exactly the written
// records and windows and the three complete arrays.
static int blkscan_host(hpk_ctx* c, const uint8_t* blocks, size_t cap, const uint32_t* block_off, uint32_t nblocks,
                        hpk_field* fields, size_t fields_cap, uint32_t* field_off, uint32_t* str_off, uint32_t* str_end,
                        size_t strs_cap, uint32_t* str_blk_off, uint8_t* status) {
    if (hpk_check_offsets(block_off, nblocks, cap)) return HPK_E_INVAL;
    if (nblocks == 0) {
        field_off[0] = 0;
        str_blk_off[0] = 0;
        return HPK_E_OK;
    }
    const uint32_t lo = block_off[0], hi = block_off[nblocks];
    const uint32_t fcap = hpk_clamp_u32(fields_cap < hi - lo ? fields_cap : hi - lo);  // (a field and a string take an
    const uint32_t scap = hpk_clamp_u32(strs_cap < hi - lo ? strs_cap : hi - lo);      // octet or more each)
    const hpk_lay_blkscan l = hpk_layout_blkscan(hi, nblocks, fcap, scap);
    hpk_slot* s;
    int rc;
    if ((rc = hpk_slot_acquire(c, &s)) ||
        (rc = hpk_slot_reserve(c, s, {{&s->bs_meta, 8 * (size_t)nblocks}, {&s->pk_tmp, hpk_pack_tmp_bytes(nblocks)}, {&s->bs_stage, l.bytes}})))
        return rc;
    const hpk_stage g{c->stream, s->bs_stage.as<uint8_t>()};
    HIP_TRY(g.up_range(l.in, blocks, lo, hi));
    HIP_TRY(g.up(l.boff, block_off, (size_t)nblocks + 1));
    if ((rc = blkscan_counts(c, s, g(l.in), hi, g(l.boff), nblocks, g(l.foff), g(l.soff), g(l.st))) ||
        (rc = hpk_launch_blkemit(c, g(l.in), hi, g(l.boff), nblocks, g(l.foff), g(l.soff), g(l.fields), fcap, g(l.so), g(l.se), scap)))
        return rc;
    HIP_TRY(g.back(field_off, l.foff, (size_t)nblocks + 1));
    HIP_TRY(g.back(str_blk_off, l.soff, (size_t)nblocks + 1));
    HIP_TRY(g.back(status, l.st, nblocks));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t nf = field_off[nblocks], ns = str_blk_off[nblocks];
    const size_t gf = nf < fcap ? nf : fcap, gs = ns < scap ? ns : scap;
    HIP_TRY(g.back(fields, l.fields, gf));
    HIP_TRY(g.back(str_off, l.so, gs));
    HIP_TRY(g.back(str_end, l.se, gs));
    if (gf || gs) HIP_TRY(hipStreamSynchronize(c->stream));
    if ((rc = hpk_slot_commit(c, s)) || (rc = hpk_take_err(c))) return rc;
    if (nf > fields_cap) return hpk_set_err_msg("the field records pass fields_cap", HPK_E_NOSPACE);
    if (ns > strs_cap) return hpk_set_err_msg("the string windows pass strs_cap", HPK_E_NOSPACE);
    return HPK_E_OK;
}

// The header-block scan (include/hpk.h).
extern "C" int hpk_scan_blocks(hpk_ctx* c, const uint8_t* blocks, size_t cap, const uint32_t* block_off, uint32_t nblocks,
                               hpk_field* fields, size_t fields_cap, uint32_t* field_off, uint32_t* str_off,
                               uint32_t* str_end, size_t strs_cap, uint32_t* str_blk_off, uint8_t* status, int flags) {
    if (!c || !block_off || !field_off || !str_blk_off || (nblocks && !status)) return hpk_set_err_msg("null argument", HPK_E_INVAL);
    if (nblocks >= 0x7FFFFFFFu) return hpk_set_err_msg("too many blocks for the block scan", HPK_E_INVAL);
    if (cap > HPK_MAX_OFFSET) return hpk_set_err_msg("the block scan's blob passes HPK_MAX_OFFSET", HPK_E_INVAL);
    if (nblocks && ((!blocks && cap) || (!fields && fields_cap) || ((!str_off || !str_end) && strs_cap)))
        return hpk_set_err_msg("null blob or list", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    if (!(flags & HPK_PTR_DEVICE))
        return blkscan_host(c, blocks, cap, block_off, nblocks, fields, fields_cap, field_off, str_off, str_end, strs_cap,
                            str_blk_off, status);
    if (((uintptr_t)fields & 15u) != 0) return hpk_set_err_msg("fields must be 16-byte aligned", HPK_E_INVAL);
    if (nblocks == 0) {
        HIP_TRY(hipMemsetAsync(field_off, 0, 4, c->stream));
        HIP_TRY(hipMemsetAsync(str_blk_off, 0, 4, c->stream));
        return blkscan_end(c, field_off, fields_cap, str_blk_off, strs_cap, flags);
    }
    hpk_slot* s;
    int rc;
    if ((rc = hpk_slot_acquire(c, &s)) ||
        (rc = hpk_slot_reserve(c, s, {{&s->bs_meta, 8 * (size_t)nblocks + 16}, {&s->pk_tmp, hpk_pack_tmp_bytes(nblocks)}})))
        return rc;
    // (a blob or a list of no capacity: an address that exists for the kernels' base pointers; nothing of it is touched)
    if (!blocks || !cap) blocks = s->bs_meta.as<uint8_t>(), cap = 0;
    if (!fields_cap) fields = reinterpret_cast<hpk_field*>(s->bs_meta.p);
    if (!strs_cap) str_off = str_end = s->bs_meta.as<uint32_t>();
    if ((rc = blkscan_counts(c, s, blocks, (uint32_t)cap, block_off, nblocks, field_off, str_blk_off, status)) ||
        (rc = hpk_launch_blkemit(c, blocks, (uint32_t)cap, block_off, nblocks, field_off, str_blk_off, fields,
                                 hpk_clamp_u32(fields_cap), str_off, str_end, hpk_clamp_u32(strs_cap))))
        return rc;
    if ((rc = hpk_slot_commit(c, s))) return rc;
    return blkscan_end(c, field_off + nblocks, fields_cap, str_blk_off + nblocks, strs_cap, flags);
}

// The static records in device memory, uploaded once per context.
static int apply_static(hpk_ctx* c) {
    if (c->d_static) return HPK_E_OK;
    const hpk_header* ent = nullptr;
    (void)hpk_static_table(nullptr, nullptr, &ent);
    hpk_header* d = nullptr;
    HIP_TRY(hipMalloc(&d, 61 * sizeof(hpk_header)));
    const hipError_t e = hipMemcpy(d, ent, 61 * sizeof(hpk_header), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return hpk_set_err("upload the static table", e);
    }
    c->d_static = d;
    return HPK_E_OK;
}

// The header-block apply (include/hpk.h).
extern "C" int hpk_apply_blocks(hpk_ctx* c, const hpk_field* fields, const uint32_t* field_off, uint32_t nblocks,
                                const uint32_t* str_out_off, const uint32_t* str_out_len, const uint8_t* str_status, uint32_t nstrs,
                                uint32_t str_base, uint32_t static_base, const uint32_t* dec_blk_off, const uint32_t* dec_blk,
                                uint32_t ndecs, hpk_dtab* tabs, hpk_header* tab_ent, size_t tab_ent_cap, hpk_header* headers,
                                size_t headers_cap, hpk_block_result* results, int flags) {
    if (!c || (nblocks && !results)) return hpk_set_err_msg("null argument", HPK_E_INVAL);
    if (!(flags & HPK_PTR_DEVICE)) return hpk_set_err_msg("the block apply takes device pointers only", HPK_E_INVAL);
    if (nblocks >= 0x7FFFFFFFu || ndecs >= 0x7FFFFFFFu) return hpk_set_err_msg("too many blocks for the block apply", HPK_E_INVAL);
    if ((((uintptr_t)fields | (uintptr_t)headers | (uintptr_t)tab_ent) & 15u) != 0)
        return hpk_set_err_msg("fields, headers and tab_ent must be 16-byte aligned", HPK_E_INVAL);
    size_t static_len = 0;
    (void)hpk_static_table(nullptr, &static_len, nullptr);
    if ((uint64_t)static_base + static_len > (1ull << 32)) return hpk_set_err_msg("the static text would pass 2^32", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    if (nblocks) HIP_TRY(hipMemsetAsync(results, 0, (size_t)nblocks * sizeof(hpk_block_result), c->stream));
    if (ndecs == 0 || nblocks == 0) return hpk_call_end(c, flags);
    if (!field_off || !dec_blk_off || !dec_blk || !tabs || (headers_cap && (!fields || !headers)) || (tab_ent_cap && !tab_ent) ||
        (nstrs && (!str_out_off || !str_out_len || !str_status)))
        return hpk_set_err_msg("null array", HPK_E_INVAL);
    if (int rc = apply_static(c)) return rc;
    if (int rc = hpk_launch_blkapply(c, fields, field_off, nblocks, str_out_off, str_out_len, str_status, nstrs, str_base, static_base,
                                     dec_blk_off, dec_blk, ndecs, tabs, tab_ent, tab_ent_cap, headers, hpk_clamp_u32(headers_cap),
                                     results, c->d_static))
        return rc;
    if (flags & HPK_ASYNC) return HPK_E_OK;
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, field_off + nblocks, 4, hipMemcpyDeviceToHost, c->stream));
    if (int rc = hpk_call_end(c, flags)) return rc;
    if ((size_t)total > headers_cap) return hpk_set_err_msg("the field total passes headers_cap", HPK_E_NOSPACE);
    return HPK_E_OK;
}

// The header-block plan (include/hpk.h).
extern "C" int hpk_plan_blocks(hpk_ctx* c, uint8_t* arena, size_t arena_cap, uint32_t static_base, uint32_t fields_base,
                               uint32_t prefix_base, const uint32_t* field_off, const uint32_t* hdr_off, uint32_t nblocks,
                               size_t hdrs_cap, const uint32_t* enc_blk_off, const uint32_t* enc_blk, const uint8_t* enc_flags,
                               uint32_t nencs, hpk_dtab* tabs, hpk_header* tab_ent, size_t tab_ent_cap, hpk_hrep* reps,
                               uint32_t* item_off, uint32_t* item_len, uint8_t* item_policy, int flags) {
    if (!c) return hpk_set_err_msg("null argument", HPK_E_INVAL);
    if (!(flags & HPK_PTR_DEVICE)) return hpk_set_err_msg("the block plan takes device pointers only", HPK_E_INVAL);
    if (arena_cap > HPK_MAX_OFFSET) return hpk_set_err_msg("the arena passes HPK_MAX_OFFSET", HPK_E_INVAL);
    if (nblocks >= 0x7FFFFFFFu || nencs >= 0x7FFFFFFFu || hdrs_cap >= 0x40000000u)
        return hpk_set_err_msg("too many blocks or headers for the block plan", HPK_E_INVAL);
    if ((((uintptr_t)reps | (uintptr_t)tab_ent) & 15u) != 0) return hpk_set_err_msg("reps and tab_ent must be 16-byte aligned", HPK_E_INVAL);
    if ((prefix_base & 3u) || (((uintptr_t)arena + prefix_base) & 3u) || (uint64_t)prefix_base + 4u * (uint64_t)hdrs_cap > arena_cap)
        return hpk_set_err_msg("the prefix area must be 4-byte aligned and inside the arena", HPK_E_INVAL);
    size_t static_len = 0;
    (void)hpk_static_table(nullptr, &static_len, nullptr);
    if ((uint64_t)static_base + static_len > arena_cap) return hpk_set_err_msg("the static text must lie inside the arena", HPK_E_INVAL);
    if (hdrs_cap && (!arena || !field_off || !reps || !item_off || !item_len || !item_policy))
        return hpk_set_err_msg("null array", HPK_E_INVAL);
    const bool plan = nencs && nblocks;
    if (plan && (!arena || !hdr_off || !enc_blk_off || !enc_blk || !enc_flags || !tabs || (tab_ent_cap && !tab_ent)))
        return hpk_set_err_msg("null array", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    if (!hdrs_cap && !plan) return hpk_call_end(c, flags);
    int rc;
    if (plan && (rc = apply_static(c))) return rc;
    hpk_slot* s = nullptr;
    if ((rc = hpk_slot_acquire(c, &s)) || (rc = hpk_slot_reserve(c, s, {{&s->bp_hash, 8 * hdrs_cap + 8}}))) return rc;
    if ((rc = hpk_launch_blkplan(c, arena, (uint32_t)arena_cap, static_base, fields_base, prefix_base, field_off, hdr_off, nblocks,
                                 (uint32_t)hdrs_cap, enc_blk_off, enc_blk, enc_flags, plan ? nencs : 0u, tabs, tab_ent, tab_ent_cap, reps,
                                 item_off, item_len, item_policy, s->bp_hash.p, c->d_static)))
        return rc;
    if ((rc = hpk_slot_commit(c, s))) return rc;
    return hpk_call_end(c, flags);
}

// The block encoder's device-plan path (hpk_henc.cpp, HPK_BLOCK_PLAN_DEVICE; not in the C ABI): the caller has
// checked the inputs, so a void encoder here is a failure. One upload of the arena below the prefix area and of the
// records; the two plan kernels; the ordered pack of the 3 nh items into a contiguous blob;
// hpk_encode_strings_packed's steps with the item policies; the offsets at the block boundaries; then the tables,
// their entries and the boundaries come back (the one wait before the end), and with the total known, exactly the bytes.
int hpk_plan_device(hpk_ctx* c, hpk_planjob* job) {
    job->bytes = nullptr;
    job->us_up = job->us_plan = job->us_items = job->us_strings = job->us_back = 0;
    const uint32_t nh = job->nh, ni = 3u * nh, nb = job->nblocks, ne = job->nencs;
    const uint64_t arena_cap = (uint64_t)job->prefix_base + 4ull * nh;
    const uint64_t in_cap = (uint64_t)job->field_off[2 * (size_t)nh] + 4ull * nh, out_cap = in_cap + 6ull * ni;
    if (!nh || !nb || !ne || nh >= 0x20000000u || arena_cap > HPK_MAX_OFFSET || out_cap > HPK_MAX_OFFSET)
        return hpk_set_err_msg("the block plan's arena or items pass the u32 offset range", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    static const bool timing = getenv("HPK_HENC_TIMING") != nullptr;
    const hpk_lay_plan l = hpk_layout_plan(arena_cap, nh, nb, ne, job->nent, in_cap, out_cap);
    const size_t tmp = hpk_pack_tmp_bytes(ni);
    hpk_slot* s;
    int rc;
    if ((rc = apply_static(c)) || (rc = hpk_slot_acquire(c, &s)) ||
        (rc = hpk_slot_reserve(c, s, {{&s->bp_hash, 8 * (size_t)nh + 8}, {&s->pk_tmp, tmp + 32}, {&s->bp_buf, l.bytes}})))
        return rc;
    stopwatch w;
    auto lap = [&](long* us) {
        if (timing) (void)hipStreamSynchronize(c->stream);
        *us = w.lap();
    };
    const hpk_stage g{c->stream, s->bp_buf.as<uint8_t>()};
    HIP_TRY(g.up(l.arena, job->arena, job->prefix_base));
    HIP_TRY(g.up(l.foff, job->field_off, 2 * (size_t)nh + 1));
    HIP_TRY(g.up(l.hoff, job->hdr_off, (size_t)nb + 1));
    HIP_TRY(g.up(l.eoff, job->enc_blk_off, (size_t)ne + 1));
    HIP_TRY(g.up(l.eblk, job->enc_blk, job->enc_blk_off[ne]));
    HIP_TRY(g.up(l.flag, job->enc_flags, ne));
    HIP_TRY(g.up(l.tabs, job->tabs, ne));
    HIP_TRY(g.up(l.ent, job->tab_ent, job->nent));
    lap(&job->us_up);
    if ((rc = hpk_launch_blkplan(c, g(l.arena), (uint32_t)arena_cap, 0u, job->fields_base, job->prefix_base, g(l.foff), g(l.hoff), nb,
                                 nh, g(l.eoff), g(l.eblk), g(l.flag), ne, g(l.tabs), g(l.ent), job->nent, g(l.reps), g(l.ioff),
                                 g(l.ilen), g(l.ipol), s->bp_hash.p, c->d_static)))
        return rc;
    lap(&job->us_plan);
    if ((rc = hpk_pack_launch(c, g(l.arena), (uint32_t)arena_cap, g(l.ioff), g(l.ilen), ni, g(l.in), (uint32_t)in_cap, g(l.inoff),
                              s->pk_tmp.p, in_cap)))
        return rc;
    lap(&job->us_items);
    if ((rc = hpk_strings_steps(c, s, tmp, g(l.in), (uint32_t)in_cap, g(l.inoff), ni, g(l.ipol), g(l.out), (uint32_t)out_cap, g(l.ooff),
                                g(l.olen), g(l.st))) ||
        (rc = hpk_launch_blkplan_boff(c, g(l.ooff), g(l.hoff), nb, g(l.boff))))
        return rc;
    lap(&job->us_strings);
    HIP_TRY(g.back(job->tabs, l.tabs, ne));
    HIP_TRY(g.back(job->tab_ent, l.ent, job->nent));
    HIP_TRY(g.back(job->block_off, l.boff, (size_t)nb + 1));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t total = job->block_off[nb];
    uint8_t* bytes = static_cast<uint8_t*>(malloc(total ? total : 1));
    if (!bytes) return hpk_set_err_msg("out of memory", HPK_E_INVAL);
    hipError_t e = total > out_cap ? hipErrorInvalidValue : hipSuccess;
    if (e == hipSuccess) e = g.back(bytes, l.out, total);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        free(bytes);
        return hpk_set_err("the planned blocks' bytes", e);
    }
    if ((rc = hpk_slot_commit(c, s)) || (rc = hpk_take_err(c))) {
        free(bytes);
        return rc;
    }
    lap(&job->us_back);
    job->bytes = bytes;
    return HPK_E_OK;
}

// The block decoder's device-scan path (hpk_hdec.cpp, HPK_BLOCK_SCAN_DEVICE; not in the C ABI): block_off is
// non-decreasing (the caller's check). The blocks and block_off go up once as they are; the count pass and the
// scans run and the two totals come back (the pipeline's one wait before its end); the outputs are sized by them;
// the emit pass and hpk_decode_strings_packed's steps over every listed string follow; then the field records,
// field_off and the strings' out_off / out_len / status come back into the context's page-locked area, and with
// out_off's last entry known, exactly the packed bytes. Everything is on the host when this returns HPK_E_OK.
int hpk_blocks_device(hpk_ctx* c, const uint8_t* blocks, const uint32_t* block_off, uint32_t nblocks, hpk_blkdev* o,
                      hpk_applyplan* plan) {
    *o = hpk_blkdev{};
    if (nblocks == 0) return HPK_E_OK;
    if (nblocks >= 0x7FFFFFFFu) return hpk_set_err_msg("too many blocks for the block scan", HPK_E_INVAL);
    const uint32_t lo = block_off[0], hi = block_off[nblocks];
    if (hi > HPK_MAX_OFFSET) return hpk_set_err_msg("the blocks pass HPK_MAX_OFFSET", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    const stopwatch w_0;
    const hpk_lay_blkhead lh = hpk_layout_blkhead(hi, nblocks);
    hpk_slot* s;
    int rc;
    if ((rc = hpk_slot_acquire(c, &s)) ||
        (rc = hpk_slot_reserve(c, s, {{&s->bs_meta, 8 * (size_t)nblocks}, {&s->pk_tmp, hpk_pack_tmp_bytes(nblocks)}, {&s->bs_stage, lh.bytes}})))
        return rc;
    const hpk_stage g{c->stream, s->bs_stage.as<uint8_t>()};
    HIP_TRY(g.up_range(lh.in, blocks, lo, hi));
    HIP_TRY(g.up(lh.boff, block_off, (size_t)nblocks + 1));
    if ((rc = blkscan_counts(c, s, g(lh.in), hi, g(lh.boff), nblocks, g(lh.foff), g(lh.soff), g(lh.st)))) return rc;
    uint32_t tot[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&tot[0], g(lh.foff) + nblocks, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&tot[1], g(lh.soff) + nblocks, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint32_t nf = tot[0], ns = tot[1];
    o->us_scan = w_0.us();
    const stopwatch w_1;
    // the outputs, sized by the totals; the strings decode to no more than the blocks' decoded bound
    const uint64_t need = (uint64_t)hpk_decoded_bound(hi) + 4ull * ns;
    if (need > HPK_MAX_OFFSET) return hpk_set_err_msg("the blocks' strings would pass 4 GiB", HPK_E_INVAL);
    const uint32_t dcap = (uint32_t)hpk_decoded_bound(hi) + 16u;
    const hpk_lay_blkout lq = hpk_layout_blkout(nf, ns, dcap);
    hpk_strdec_scratch k{};
    if ((rc = hpk_slot_reserve(c, s, {{&s->bs_out, lq.bytes}}))) return rc;
    if (ns && (rc = hpk_strdec_reserve(c, s, hi, ns, need, 0, &k))) return rc;
    const hpk_stage q{c->stream, s->bs_out.as<uint8_t>()};
    if ((rc = hpk_launch_blkemit(c, g(lh.in), hi, g(lh.boff), nblocks, g(lh.foff), g(lh.soff), q(lq.fields), nf, q(lq.so), q(lq.se), ns)))
        return rc;
    if (ns && (rc = hpk_strdec_steps(c, s, k, need, g(lh.in), hi, q(lq.so), q(lq.se), ns, q(lq.out), dcap, q(lq.oo), q(lq.ol), nullptr,
                                     q(lq.ss))))
        return rc;
    // back into the page-locked area (with a plan, the apply's outputs behind the rest)
    const size_t nd = plan ? plan->ndecs : 0, ne = plan ? plan->nent : 0;
    const hpk_lay_blkpin lp = hpk_layout_blkpin(nf, nblocks, ns, dcap, plan != nullptr, nd, ne);
    uint8_t* h = nullptr;
    if ((rc = hpk_ctx_pinned(c, lp.bytes, (void**)&h))) return rc;
    if (plan) {
        // HPK_BLOCK_APPLY_DEVICE: the lists and the tables go up, hpk_apply_blocks' kernel runs on what the steps
        // above left on the device, and the results, the tables' records and the strings' total come back. Nothing
        // deferred: the header records, the tables' entries and exactly the packed bytes follow, and the field
        // records and the strings' arrays stay where they are. Else the call goes on as without a plan.
        const stopwatch w_a;
        plan->applied = 0;
        const hpk_lay_blkapply la = hpk_layout_blkapply(nd, nblocks, ne, nf);
        if ((rc = hpk_slot_reserve(c, s, {{&s->ba_buf, la.bytes}})) || (rc = apply_static(c))) return rc;
        const hpk_stage a{c->stream, s->ba_buf.as<uint8_t>()};
        HIP_TRY(a.up(la.doff, plan->dec_blk_off, nd + 1));
        HIP_TRY(a.up(la.blk, plan->dec_blk, nblocks));
        HIP_TRY(a.up(la.tabs, plan->tabs, nd));
        HIP_TRY(a.up(la.ent, plan->tab_ent, ne));
        HIP_TRY(hipMemsetAsync(a(la.res), 0, la.zeroed, c->stream));  // the results and the header records
        if ((rc = hpk_launch_blkapply(c, q(lq.fields), g(lh.foff), nblocks, q(lq.oo), q(lq.ol), q(lq.ss), ns, plan->str_base, 0u, a(la.doff),
                                      a(la.blk), plan->ndecs, a(la.tabs), a(la.ent), ne, a(la.hdr), nf, a(la.res), c->d_static)))
            return rc;
        uint32_t total = 0;
        HIP_TRY(a.back(lp.res.in(h), la.res, nblocks));
        HIP_TRY(a.back(lp.tabs.in(h), la.tabs, nd));
        if (ns) HIP_TRY(hipMemcpyAsync(&total, q(lq.oo) + ns, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if ((rc = hpk_take_err(c))) return rc;  // (a void decoder: the lists or the tables the host made are wrong)
        const hpk_dtab* tb = lp.tabs.in(h);
        bool deferred = false;
        for (size_t k = 0; k < nd; ++k) deferred |= tb[k].applied != plan->dec_blk_off[k + 1] - plan->dec_blk_off[k];
        plan->us_apply = w_a.us();
        if (!deferred) {
            if (total > dcap) return hpk_set_err_msg("the blocks' strings pass their decoded bound", HPK_E_DEVICE);
            HIP_TRY(a.back(lp.hdr.in(h), la.hdr, nf));
            HIP_TRY(a.back(lp.ent.in(h), la.ent, ne));
            HIP_TRY(q.back(lp.out.in(h), lq.out, total));
            HIP_TRY(hipStreamSynchronize(c->stream));
            if ((rc = hpk_slot_commit(c, s))) return rc;
            plan->applied = 1;
            plan->results = lp.res.in(h);
            plan->tabs_out = tb;
            plan->headers = lp.hdr.in(h);
            plan->ent_out = lp.ent.in(h);
            plan->packed_len = total;
            o->arena = lp.out.in(h);
            o->nfields = nf;
            o->nstrs = ns;
            o->us_strings = w_1.us();
            return HPK_E_OK;
        }
    }
    HIP_TRY(q.back(lp.fields.in(h), lq.fields, nf));
    HIP_TRY(g.back(lp.foff.in(h), lh.foff, (size_t)nblocks + 1));
    uint32_t* h_off = lp.oo.in(h);
    h_off[0] = 0;
    if (ns) {
        HIP_TRY(q.back(h_off, lq.oo, (size_t)ns + 1));
        HIP_TRY(q.back(lp.ol.in(h), lq.ol, ns));
        HIP_TRY(q.back(lp.ss.in(h), lq.ss, ns));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    o->us_strings = w_1.us();
    const stopwatch w_2;
    const uint32_t total = h_off[ns];
    if (total > dcap) return hpk_set_err_msg("the blocks' strings pass their decoded bound", HPK_E_DEVICE);
    if (total) {
        HIP_TRY(q.back(lp.out.in(h), lq.out, total));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if ((rc = hpk_slot_commit(c, s))) return rc;
    o->fields = lp.fields.in(h);
    o->field_off = lp.foff.in(h);
    o->out_off = h_off;
    o->out_len = lp.ol.in(h);
    o->status = lp.ss.in(h);
    o->arena = lp.out.in(h);
    o->nfields = nf;
    o->nstrs = ns;
    o->us_back = w_2.us();
    return HPK_E_OK;
}
