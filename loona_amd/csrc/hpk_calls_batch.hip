// hpk_calls_batch.hip — the batch entry points of the C ABI (include/hpk.h): the region, compacted and packed
// decodes, the pack, the encodes, and the chunked pipeline of the host-pointer batches.
#include "hpk_calls.h"

int hpk_check_offsets(const uint32_t* off, uint32_t n, size_t cap) {
    for (uint32_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return hpk_set_err_msg("offsets must be non-decreasing", HPK_E_INVAL);
    if (off[n] > cap || off[n] > HPK_MAX_OFFSET) return hpk_set_err_msg("offsets pass the blob's capacity", HPK_E_INVAL);
    return HPK_E_OK;
}

uint32_t hpk_clamp_cap(size_t cap) { return cap > HPK_MAX_OFFSET ? HPK_MAX_OFFSET : (uint32_t)cap; }
uint32_t hpk_clamp_u32(size_t x) { return x > 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)x; }

int hpk_call_end(hpk_ctx* c, int flags) {
    if (flags & HPK_ASYNC) return HPK_E_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return hpk_take_err(c);
}

typedef int (*launch_fn)(hpk_ctx*, const hpk_batch&);

// the region form's decode as a launch_fn: the stream's slot with its list, the launch, the slot used
static int decode_region(hpk_ctx* c, const hpk_batch& b) {
    hpk_slot* s;
    int rc;
    if ((rc = hpk_slot_acquire(c, &s)) || (rc = hpk_slot_reserve(c, s, {{&s->long_list, 4 * (size_t)b.n}}))) return rc;
    if ((rc = hpk_launch_decode(c, b, s->long_list.as<uint32_t>()))) return rc;
    return hpk_slot_commit(c, s);
}

// Host-pointer batches: stage, run and copy back, cut into up to kMaxChunks literal ranges balanced
// by encoded bytes; chunk j's copy-in (h2d stream), kernel (ctx stream) and copy-out (d2h stream)
// overlap with the neighbouring chunks' (PCIe is full duplex), and ev_out[j] marks its results in
// host memory. Offsets stay absolute, so every chunk is the same kernel on a sub-range of the
// scratch buffers. With pageable host memory HIP stages the copies itself and the overlap is small:
// register the arena (hpk_host_register). `trusted`: the offsets were made by the library itself
// (hpk_hdec_decode_blocks), monotone by construction, so the O(n) host checks are skipped.
static int queue_chunks(launch_fn fn, hpk_ctx* c, const uint8_t* in_blob, const uint32_t* in_off, uint8_t* out_blob,
                        const uint32_t* out_off, uint32_t* out_len, uint8_t* status, uint32_t n, size_t in_bytes,
                        size_t out_bytes, int chunks, const uint32_t* cut, uint32_t* d_in_off, uint32_t* d_out_off,
                        uint32_t* d_len);

static int host_begin(launch_fn fn, hpk_ctx* c, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off,
                      uint32_t n, uint8_t* out_blob, size_t out_cap, const uint32_t* out_off, uint32_t* out_len,
                      uint8_t* status, bool trusted, int* nchunks, uint32_t* cut) {
    *nchunks = 0;
    if (!trusted && (hpk_check_offsets(in_off, n, in_cap) || hpk_check_offsets(out_off, n, out_cap))) return HPK_E_INVAL;
    if (n == 0) return HPK_E_OK;
    const size_t in_bytes = in_off[n], out_bytes = out_off[n];
    if ((in_bytes && !in_blob) || (out_bytes && !out_blob)) return hpk_set_err_msg("null blob", HPK_E_INVAL);
    int rc;
    if ((rc = hpk_grow((void**)&c->d_in, &c->d_in_cap, in_bytes + 16))) return rc;
    if ((rc = hpk_grow((void**)&c->d_out, &c->d_out_cap, out_bytes + 16))) return rc;
    if ((rc = hpk_grow((void**)&c->d_meta, &c->d_meta_cap, (3 * (size_t)n + 2) * 4))) return rc;
    if ((rc = hpk_grow((void**)&c->d_st, &c->d_st_cap, n))) return rc;
    uint32_t* d_in_off = c->d_meta;
    uint32_t* d_out_off = c->d_meta + (n + 1);
    uint32_t* d_len = c->d_meta + 2 * ((size_t)n + 1);
    if (!c->h2d) {
        HIP_TRY(hipStreamCreateWithFlags(&c->h2d, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&c->d2h, hipStreamNonBlocking));
        for (int j = 0; j < hpk_ctx::kMaxChunks; ++j) {
            HIP_TRY(hipEventCreateWithFlags(&c->ev_in[j], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&c->ev_run[j], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&c->ev_out[j], hipEventDisableTiming));
        }
    }
    const int chunks = hpk_chunk_cuts(in_off, n, out_bytes, cut);  // (hpk_chunks.h)
    // A failure after some chunk's copies were queued leaves DMA into and out of the caller's buffers
    // (and the pinned staging area the block decoder reuses) in flight: drain the three streams before
    // returning, so nothing lands after the call has returned.
    auto drain = [&](int rc) {
        (void)hipStreamSynchronize(c->h2d);
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamSynchronize(c->d2h);
        return rc;
    };
    if (int e = queue_chunks(fn, c, in_blob, in_off, out_blob, out_off, out_len, status, n, in_bytes, out_bytes,
                             chunks, cut, d_in_off, d_out_off, d_len))
        return drain(e);
    *nchunks = chunks;
    return HPK_E_OK;
}

static int queue_chunks(launch_fn fn, hpk_ctx* c, const uint8_t* in_blob, const uint32_t* in_off, uint8_t* out_blob,
                        const uint32_t* out_off, uint32_t* out_len, uint8_t* status, uint32_t n, size_t in_bytes,
                        size_t out_bytes, int chunks, const uint32_t* cut, uint32_t* d_in_off, uint32_t* d_out_off,
                        uint32_t* d_len) {
    int rc;
    HIP_TRY(hipEventRecord(c->ev_run[0], c->stream));  // earlier work on the ctx stream first
    HIP_TRY(hipStreamWaitEvent(c->h2d, c->ev_run[0], 0));
    for (int j = 0; j < chunks; ++j) {
        const uint32_t a = cut[j], b = cut[j + 1];
        if (a < b) {
            const size_t ib = in_off[a], ie = in_off[b], ob = out_off[a], oe = out_off[b];
            if (ie > ib) HIP_TRY(hipMemcpyAsync(c->d_in + ib, in_blob + ib, ie - ib, hipMemcpyHostToDevice, c->h2d));
            HIP_TRY(hipMemcpyAsync(d_in_off + a, in_off + a, (b - a + 1) * 4ull, hipMemcpyHostToDevice, c->h2d));
            HIP_TRY(hipMemcpyAsync(d_out_off + a, out_off + a, (b - a + 1) * 4ull, hipMemcpyHostToDevice, c->h2d));
            HIP_TRY(hipEventRecord(c->ev_in[j], c->h2d));
            HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_in[j], 0));
            const hpk_batch bt{c->d_in, (uint32_t)in_bytes, d_in_off + a, b - a, c->d_out, (uint32_t)out_bytes,
                               d_out_off + a, d_len + a, c->d_st + a};
            if ((rc = fn(c, bt))) return rc;
            HIP_TRY(hipEventRecord(c->ev_run[j], c->stream));
            HIP_TRY(hipStreamWaitEvent(c->d2h, c->ev_run[j], 0));
            if (oe > ob) HIP_TRY(hipMemcpyAsync(out_blob + ob, c->d_out + ob, oe - ob, hipMemcpyDeviceToHost, c->d2h));
            HIP_TRY(hipMemcpyAsync(out_len + a, d_len + a, (b - a) * 4ull, hipMemcpyDeviceToHost, c->d2h));
            HIP_TRY(hipMemcpyAsync(status + a, c->d_st + a, b - a, hipMemcpyDeviceToHost, c->d2h));
        }
        HIP_TRY(hipEventRecord(c->ev_out[j], c->d2h));
    }
    return HPK_E_OK;
}

static int host_end(hpk_ctx* c) {
    HIP_TRY(hipStreamSynchronize(c->d2h));
    return hpk_take_err(c);
}

static int run_batch(launch_fn fn, hpk_ctx* c, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off,
                     uint32_t n, uint8_t* out_blob, size_t out_cap, const uint32_t* out_off, uint32_t* out_len,
                     uint8_t* status, int flags) {
    if (!c || !in_off || !out_off || (n && (!out_len || !status))) return hpk_set_err_msg("null argument", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    if (flags & HPK_PTR_DEVICE) {
        if (n == 0) return HPK_E_OK;
        if (!in_blob || !out_blob) return hpk_set_err_msg("null blob", HPK_E_INVAL);
        const hpk_batch b{in_blob, hpk_clamp_cap(in_cap), in_off, n, out_blob, hpk_clamp_cap(out_cap), out_off, out_len, status};
        if (fn == decode_region && !(flags & HPK_ASYNC) && c->sm_max) {  // the small-call mode
            bool handled = false;
            if (int rc = hpk_persist_call(c, b, &handled)) return rc;
            if (handled) return HPK_E_OK;
        }
        if (int rc = fn(c, b)) return rc;
        return hpk_call_end(c, flags);
    }
    int chunks;
    uint32_t cut[hpk_ctx::kMaxChunks + 1];
    if (int rc = host_begin(fn, c, in_blob, in_cap, in_off, n, out_blob, out_cap, out_off, out_len, status, false,
                            &chunks, cut))
        return rc;
    return chunks ? host_end(c) : HPK_E_OK;
}

// The block decoder's form (hpk_hdec.cpp): a trusted host batch started here, its chunks' results
// waited for one by one (so the caller applies chunk j's blocks while later chunks still decode),
// then finished. Not part of the C ABI.
int hpk_decode_host_begin(hpk_ctx* c, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off, uint32_t n,
                          uint8_t* out_blob, size_t out_cap, const uint32_t* out_off, uint32_t* out_len,
                          uint8_t* status, int* nchunks, uint32_t* cut) {
    HIP_TRY(hipSetDevice(c->device));
    return host_begin(decode_region, c, in_blob, in_cap, in_off, n, out_blob, out_cap, out_off, out_len, status,
                      true, nchunks, cut);
}

int hpk_host_chunk_wait(hpk_ctx* c, int j) {
    HIP_TRY(hipEventSynchronize(c->ev_out[j]));
    return HPK_E_OK;
}

int hpk_decode_host_end(hpk_ctx* c) { return host_end(c); }

int hpk_ctx_max_chunks() { return hpk_ctx::kMaxChunks; }

extern "C" int hpk_decode_batch(hpk_ctx* c, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off, uint32_t n,
                                uint8_t* out_blob, size_t out_cap, const uint32_t* out_off, uint32_t* out_len,
                                uint8_t* status, int flags) {
    return run_batch(decode_region, c, in_blob, in_cap, in_off, n, out_blob, out_cap, out_off, out_len, status,
                     flags);
}

int hpk_check_call(const hpk_ctx* c, bool null_arg, int flags, uint32_t n, const char* what, const size_t* in_cap, uint64_t* need) {
    auto inval = [&](const char* before, const char* after) {
        return hpk_set_err_msg((std::string(before) + what + after).c_str(), HPK_E_INVAL);
    };
    if (!c || null_arg) return hpk_set_err_msg("null argument", HPK_E_INVAL);
    if (!(flags & HPK_PTR_DEVICE)) return inval("the ", " takes device pointers only");
    if (n >= 0x7FFFFFFFu) return inval("too many literals for the ", "");
    if (in_cap) {
        *need = (uint64_t)hpk_decoded_bound(hpk_clamp_cap(*in_cap)) + 4ull * n;
        if (*need > HPK_MAX_OFFSET) return inval("the ", "'s output would pass 4 GiB");
    }
    return HPK_E_OK;
}

// The compacted form (include/hpk.h). The kernels' images keep bound-sized regions (a literal's decoded
// length is known only once it is decoded). Wave-fill kernel (large batches): it makes the bound layout
// from in_off itself, each workgroup packing into its range's span, and writes out_off[n]. Workgroup-fill
// kernel: the bound layout made on the device by a scan of the literals' 4-rounded bounds, the output
// cursor zeroed, the kernel, then the cursor copied to out_off[n].
extern "C" int hpk_decode_batch_compact(hpk_ctx* c, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off,
                                        uint32_t n, uint8_t* out_blob, size_t out_cap, uint32_t* out_off,
                                        uint32_t* out_len, uint8_t* status, int flags) {
    uint64_t need;
    if (int rc = hpk_check_call(c, !in_off || !out_off || (n && (!out_len || !status)), flags, n, "compacted form", &in_cap,
                            &need))
        return rc;
    if (out_cap < need) return hpk_set_err_msg("out_cap below hpk_decoded_bound(in_cap) + 4 n", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(out_off, 0, 4, c->stream));
        return hpk_call_end(c, flags);
    }
    if (!in_blob || !out_blob) return hpk_set_err_msg("null blob", HPK_E_INVAL);
    const bool wave = hpk_compact_wave(c, n);
    hpk_slot* s;
    int rc;
    if ((rc = hpk_slot_acquire(c, &s))) return rc;
    if (wave)
        rc = hpk_slot_reserve(c, s, {{&s->long_list, 4 * (size_t)n}});
    else
        rc = hpk_slot_reserve(c, s, {{&s->long_list, 4 * (size_t)n}, {&s->cp_bound, 4 * ((size_t)n + 1)},
                                 {&s->cp_tmp, hpk_bound_tmp_bytes(n)}, {&s->cp_cursor, 4}});
    if (rc) return rc;
    hpk_batch b{in_blob, hpk_clamp_cap(in_cap), in_off, n, out_blob, hpk_clamp_cap(out_cap), nullptr, out_len, status};
    uint32_t* cursor = nullptr;
    if (!wave) {
        b.out_off = s->cp_bound.as<uint32_t>();
        cursor = s->cp_cursor.as<uint32_t>();
        if ((rc = hpk_bound_scan(c, in_off, n, s->cp_bound.as<uint32_t>(), s->cp_tmp.p))) return rc;
        HIP_TRY(hipMemsetAsync(cursor, 0, 4, c->stream));
    }
    if ((rc = hpk_launch_decode_compact(c, b, out_off, s->long_list.as<uint32_t>(), cursor, wave))) return rc;
    if (!wave)  // the span written: the cursor
        HIP_TRY(hipMemcpyAsync(out_off + n, cursor, 4, hipMemcpyDeviceToDevice, c->stream));
    if ((rc = hpk_slot_commit(c, s))) return rc;
    return hpk_call_end(c, flags);
}

int hpk_packed_end(hpk_ctx* c, const uint32_t* dst_off_n, size_t dst_cap, int flags) {
    if (flags & HPK_ASYNC) return HPK_E_OK;
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, dst_off_n, 4, hipMemcpyDeviceToHost, c->stream));
    if (int rc = hpk_call_end(c, flags)) return rc;
    if ((size_t)total > dst_cap) return hpk_set_err_msg("the packed bytes pass the output capacity", HPK_E_NOSPACE);
    return HPK_E_OK;
}

// The packed form (include/hpk.h): the region decode into the slot's scratch blob, laid out by the
// 4-rounded decoded bounds (hpk_bound_scan), out_len and status straight to the caller's arrays; then
// out_off = the exclusive sum of out_len and the ordered pack from the scratch to out_blob (hpk_pack.hip).
// No existing kernel changes, and the persistent kernel is not asked (always the launch path).
extern "C" int hpk_decode_batch_packed(hpk_ctx* c, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off,
                                       uint32_t n, uint8_t* out_blob, size_t out_cap, uint32_t* out_off,
                                       uint32_t* out_len, uint8_t* status, int flags) {
    uint64_t need;
    if (int rc = hpk_check_call(c, !in_off || !out_off || (n && (!out_len || !status)), flags, n, "packed form", &in_cap, &need))
        return rc;
    if (n && (!in_blob || (!out_blob && out_cap))) return hpk_set_err_msg("null blob", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    if (n == 0) return hpk_packed_empty(c, out_off, out_cap, flags);
    size_t tmp = hpk_bound_tmp_bytes(n);  // (the two scans follow each other: one scratch)
    if (tmp < hpk_pack_tmp_bytes(n)) tmp = hpk_pack_tmp_bytes(n);
    hpk_slot* s;
    int rc;
    if ((rc = hpk_slot_acquire(c, &s)) ||
        (rc = hpk_slot_reserve(c, s, {{&s->long_list, 4 * (size_t)n}, {&s->pk_bound, 4 * ((size_t)n + 1)}, {&s->pk_tmp, tmp},
                                  {&s->pk_scratch, (size_t)need + 64}})))
        return rc;
    uint32_t* bound = s->pk_bound.as<uint32_t>();
    uint8_t* scratch = s->pk_scratch.as<uint8_t>();
    if ((rc = hpk_bound_scan(c, in_off, n, bound, s->pk_tmp.p))) return rc;
    const hpk_batch b{in_blob, hpk_clamp_cap(in_cap), in_off, n, scratch, (uint32_t)need, bound, out_len, status};
    if ((rc = hpk_launch_decode(c, b, s->long_list.as<uint32_t>()))) return rc;
    if ((rc = hpk_pack_launch(c, scratch, (uint32_t)need, bound, out_len, n, out_blob, hpk_clamp_cap(out_cap), out_off,
                              s->pk_tmp.p, need)))
        return rc;
    if ((rc = hpk_slot_commit(c, s))) return rc;
    return hpk_packed_end(c, out_off + n, out_cap, flags);
}

// The pack step on its own: results already held in the region or compacted layout, laid end to end.
extern "C" int hpk_pack_batch(hpk_ctx* c, const uint8_t* src_blob, size_t src_cap, const uint32_t* src_off,
                              const uint32_t* src_len, uint32_t n, uint8_t* dst_blob, size_t dst_cap, uint32_t* dst_off,
                              int flags) {
    if (int rc = hpk_check_call(c, !dst_off || (n && (!src_off || !src_len)), flags, n, "pack", nullptr, nullptr)) return rc;
    if (n && ((!src_blob && src_cap) || (!dst_blob && dst_cap))) return hpk_set_err_msg("null blob", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    hpk_slot* s;
    int rc;
    if ((rc = hpk_slot_acquire(c, &s)) || (rc = hpk_slot_reserve(c, s, {{&s->pk_tmp, hpk_pack_tmp_bytes(n)}}))) return rc;
    if ((rc = hpk_pack_launch(c, src_blob, hpk_clamp_cap(src_cap), src_off, src_len, n, dst_blob, hpk_clamp_cap(dst_cap), dst_off,
                              s->pk_tmp.p, HPK_MAX_OFFSET)))
        return rc;
    if ((rc = hpk_slot_commit(c, s))) return rc;
    return hpk_packed_end(c, dst_off + n, dst_cap, flags);
}

extern "C" int hpk_encode_batch(hpk_ctx* c, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off, uint32_t n,
                                uint8_t* out_blob, size_t out_cap, const uint32_t* out_off, uint32_t* out_len,
                                uint8_t* status, int flags) {
    return run_batch(hpk_launch_encode, c, in_blob, in_cap, in_off, n, out_blob, out_cap, out_off, out_len, status,
                     flags);
}

// The encoded lengths alone (include/hpk.h): the length pass of the packed encode, no scratch.
extern "C" int hpk_encoded_len_batch(hpk_ctx* c, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off, uint32_t n,
                                     uint32_t* out_len, int flags) {
    if (int rc = hpk_check_call(c, !in_off || (n && !out_len), flags, n, "encoded-length call", nullptr, nullptr)) return rc;
    if (n == 0) return HPK_E_OK;
    if (!in_blob && in_cap) return hpk_set_err_msg("null blob", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    hpk_in_or_codes(c, &in_blob, &in_cap);
    if (int rc = hpk_launch_enclen(c, in_blob, hpk_clamp_cap(in_cap), in_off, n, out_len, nullptr)) return rc;
    return hpk_call_end(c, flags);
}

// The packed encode (include/hpk.h): the length pass writes out_len and status, the length scan out_off, and
// the encode kernel's packed instantiation writes every literal at its final place, clipped at out_cap. The
// only scratch is the scan's tile sums; the word after them is the scan's verdict on the total.
extern "C" int hpk_encode_batch_packed(hpk_ctx* c, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off,
                                       uint32_t n, uint8_t* out_blob, size_t out_cap, uint32_t* out_off,
                                       uint32_t* out_len, uint8_t* status, int flags) {
    if (int rc = hpk_check_call(c, !in_off || !out_off || (n && (!out_len || !status)), flags, n, "packed encode", nullptr,
                            nullptr))
        return rc;
    if (n && ((!in_blob && in_cap) || (!out_blob && out_cap))) return hpk_set_err_msg("null blob", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    if (n == 0) return hpk_packed_empty(c, out_off, out_cap, flags);
    const size_t tmp = hpk_pack_tmp_bytes(n);
    hpk_slot* s;
    int rc;
    if ((rc = hpk_slot_acquire(c, &s)) || (rc = hpk_slot_reserve(c, s, {{&s->pk_tmp, tmp + 32}}))) return rc;
    hpk_in_or_codes(c, &in_blob, &in_cap);
    hpk_out_or_tmp(s, tmp, &out_blob, &out_cap);
    if ((rc = hpk_launch_enclen(c, in_blob, hpk_clamp_cap(in_cap), in_off, n, out_len, status))) return rc;
    if ((rc = hpk_len_scan(c, out_len, n, out_off, s->pk_tmp.p))) return rc;
    const hpk_batch b{in_blob, hpk_clamp_cap(in_cap), in_off, n, out_blob, hpk_clamp_cap(out_cap), out_off, out_len, status};
    if ((rc = hpk_launch_encode_packed(c, b, hpk_len_scan_verdict(s->pk_tmp.p, n)))) return rc;
    if ((rc = hpk_slot_commit(c, s))) return rc;
    return hpk_packed_end(c, out_off + n, out_cap, flags);
}
