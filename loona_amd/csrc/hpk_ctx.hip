// hpk_ctx.hip — device context and the batch entry points of the C ABI (include/hpk.h).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>

#include <chrono>
#include <initializer_list>

#include "hpk_device.h"

#define HPK_VERSION "hpk 0.46 gfx950 decode v42 (every batch: wave fills, each wave with its own LDS window and image, lookups in a 13-bit two-symbol table, the lane loop in rounds of four nested body steps with long codes taken once a round, longest-first queue sorted under the previous image's LDS read-out, the next fill's loads issued ahead of the write-back's stores, slot end offsets by DPP, nontemporal window loads stopping at the chunk's last byte, nontemporal write-back; chunks by guided self-scheduling from 4M literals, fixed 96-literal chunks below; fills and long-literal phase: body steps with no fit tests while >= 31 bits are left (29 with the 12-bit table), then the wave fills' tails as four masked lookups with no fit test per code (checked steps only for a 14..30-bit code or a cut code in the tail), a lane's first literal's tail from the word saved where its body ended and its status carried from that tail, and the other kernels' checked tails (the long phase's at its refill points); long literals one lane each streaming from HBM after the fills, dense ranges listed longest-first; literals of >= 8 KiB by a whole workgroup in speculative pieces; compacted-output form: wave fills packed per workgroup from an LDS cursor into a bound layout made from the input offsets, each lane storing its two literals in unaligned 16-byte pieces; small-call mode: a persistent kernel behind a host-mapped doorbell); encode v5 (byte-balanced workgroup ranges, start map and DPP segmented scan, run accumulator, LDS image, live chunks only; packed form: length pass, length scan, the same kernel into exact positions; string literals v1: length pass + form step, length scan, a tile kernel that writes prefix, H bit and the Huffman or raw payload); string-literal decode v1 (parse kernel, Huffman payloads gathered by the ordered pack, the packed form's region decode, merge, length scan, ordered pack with a source per string); block scan v1 (count pass, length scans, emit pass: one lane per block); block apply v1 (one wave per decoder: lane-parallel look and stage, records resolved in order against a ring in LDS); block plan v1 (a default-and-hash pass, then one wave per encoder: headers resolved in order against a hashed ring in LDS, 64 entries a search step, matches confirmed on bytes)"

static thread_local std::string t_last_error;

int hpk_set_err(const char* what, hipError_t e) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    t_last_error = buf;
    return HPK_E_DEVICE;
}

int hpk_set_err_msg(const char* what, int code) {
    t_last_error = what;
    return code;
}


extern "C" const char* hpk_version(void) { return HPK_VERSION; }

extern "C" const char* hpk_last_error(const hpk_ctx*) { return t_last_error.c_str(); }

extern "C" hpk_ctx* hpk_ctx_create(int device) {
    const hpk_tables* t = hpk_get_tables();
    if (!t) { hpk_set_err_msg("code table build failed", HPK_E_INVAL); return nullptr; }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) { hpk_set_err("hipGetDeviceCount", e); return nullptr; }
    if (device < 0 || device >= ndev) { hpk_set_err_msg("device index out of range", HPK_E_INVAL); return nullptr; }
    hpk_ctx* c = new hpk_ctx();
    c->device = device;
    auto fail = [&](const char* what, hipError_t err) {
        hpk_set_err(what, err);
        hpk_ctx_destroy(c);
        return (hpk_ctx*)nullptr;
    };
    if ((e = hipSetDevice(device)) != hipSuccess) return fail("hipSetDevice", e);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return fail("hipGetDeviceProperties", e);
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        hpk_set_err_msg("libhpk kernels are built for gfx950 only", HPK_E_NODEVICE);
        delete c;
        return nullptr;
    }
    c->num_cu = prop.multiProcessorCount;
    if ((e = hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e);
    c->stream = c->own;
    if ((e = hipMalloc(&c->d_lut2, sizeof(t->lut2))) != hipSuccess) return fail("hipMalloc lut2", e);
    if ((e = hipMemcpy(c->d_lut2, t->lut2, sizeof(t->lut2), hipMemcpyHostToDevice)) != hipSuccess)
        return fail("upload lut2", e);
    if ((e = hipMalloc(&c->d_lut3, sizeof(t->lut3))) != hipSuccess) return fail("hipMalloc lut3", e);
    if ((e = hipMemcpy(c->d_lut3, t->lut3, sizeof(t->lut3), hipMemcpyHostToDevice)) != hipSuccess)
        return fail("upload lut3", e);
    if ((e = hipMalloc(&c->d_lut13, sizeof(t->lut13))) != hipSuccess) return fail("hipMalloc lut13", e);
    if ((e = hipMemcpy(c->d_lut13, t->lut13, sizeof(t->lut13), hipMemcpyHostToDevice)) != hipSuccess)
        return fail("upload lut13", e);
    if ((e = hipMalloc(&c->d_lo, sizeof(t->lo))) != hipSuccess) return fail("hipMalloc lo", e);
    if ((e = hipMalloc(&c->d_codes, 2 * 257 * sizeof(uint32_t))) != hipSuccess) return fail("hipMalloc codes", e);
    uint32_t packed[2 * 257];
    for (int s = 0; s < 257; ++s) {
        packed[s] = t->code[s];
        packed[257 + s] = t->len[s];
    }
    if ((e = hipMemcpy(c->d_lo, t->lo, sizeof(t->lo), hipMemcpyHostToDevice)) != hipSuccess) return fail("upload lo", e);
    if ((e = hipMemcpy(c->d_codes, packed, sizeof(packed), hipMemcpyHostToDevice)) != hipSuccess) return fail("upload codes", e);
    if ((e = hipHostMalloc((void**)&c->h_err, 64, hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess)
        return fail("hipHostMalloc err flag", e);
    *c->h_err = 0;
    if ((e = hipHostGetDevicePointer((void**)&c->d_err, c->h_err, 0)) != hipSuccess) return fail("err flag pointer", e);
    return c;
}

static int grow(void** p, size_t* cap, size_t need) {
    if (need <= *cap) return HPK_E_OK;
    size_t n = need + need / 4 + 4096;
    (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    HIP_TRY(hipMalloc(p, n));
    *cap = n;
    return HPK_E_OK;
}

// The per-stream slots: hpk_slot (hpk_device.h) has the rules these three keep.
// slot_acquire: the slot of the context's current stream, claimed or taken over if it has none.
static int slot_acquire(hpk_ctx* c, hpk_slot** slot) {
    hpk_slot* s = nullptr;
    bool any = false;
    for (hpk_slot& k : c->slots) {
        if (k.used && k.stream == c->stream) s = &k;
        any |= k.used;
    }
    if (!s) {
        if (any && !c->slot_events) {  // a second stream: events from here on; the past is drained once,
            // here. (Recording an event on each earlier slot's stream would touch a handle the caller may
            // have destroyed since.) The only slots without an event were used on the own stream.
            c->slot_events = true;
            HIP_TRY(hipStreamSynchronize(c->own));
            for (hpk_slot& k : c->slots)
                if (k.stream == c->own) k.ev_set = false;
        }
        int j = 0;
        while (j < hpk_ctx::kSlots && c->slots[j].used) ++j;
        if (j == hpk_ctx::kSlots) {  // all taken: the oldest, once its last launch is done
            j = c->slot_next;
            c->slot_next = (j + 1) % hpk_ctx::kSlots;
            if (c->slots[j].ev_set) HIP_TRY(hipEventSynchronize(c->slots[j].ev));
        }
        s = &c->slots[j];
        s->stream = c->stream;
    }
    if (c->slot_events && !s->ev) HIP_TRY(hipEventCreateWithFlags(&s->ev, hipEventDisableTiming));
    *slot = s;
    return HPK_E_OK;
}

// slot_reserve: the buffers a call is about to use, each of at least its bytes. If any must grow, the
// slot's last launch is waited for first (once), through its event or else the own stream.
struct slot_need {
    DevBuf* buf;
    size_t bytes;
};
static int slot_reserve(hpk_ctx* c, hpk_slot* s, std::initializer_list<slot_need> needs) {
    bool small = false;
    for (const slot_need& nd : needs) small |= nd.buf->cap < nd.bytes;
    if (small) {
        if (s->ev_set)
            HIP_TRY(hipEventSynchronize(s->ev));
        else if (s->used)
            HIP_TRY(hipStreamSynchronize(c->own));
        for (const slot_need& nd : needs)
            if (int rc = grow(&nd.buf->p, &nd.buf->cap, nd.bytes)) return rc;
    }
    s->used = true;
    return HPK_E_OK;
}

// slot_commit: after the call's last operation on the stream, the slot's event recorded there.
static int slot_commit(hpk_ctx* c, hpk_slot* s) {
    if (!c->slot_events && c->stream == c->own) return HPK_E_OK;
    if (!s->ev) HIP_TRY(hipEventCreateWithFlags(&s->ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(s->ev, c->stream));
    s->ev_set = true;
    return HPK_E_OK;
}

extern "C" void hpk_ctx_destroy(hpk_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hpk_persist_stop(c);
    if (c->sm_stream) (void)hipStreamDestroy(c->sm_stream);
    if (c->h_sm) (void)hipHostFree(c->h_sm);
    (void)hipFree(c->d_sm_dev);
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(c->d_lut2);
    (void)hipFree(c->d_lut3);
    (void)hipFree(c->d_lut13);
    (void)hipFree(c->d_lo);
    (void)hipFree(c->d_codes);
    (void)hipFree(c->d_static);
    (void)hipFree(c->d_in);
    (void)hipFree(c->d_out);
    (void)hipFree(c->d_meta);
    (void)hipFree(c->d_st);
    if (c->h_err) (void)hipHostFree(c->h_err);
    if (c->h_pin) (void)hipHostFree(c->h_pin);
    for (hpk_slot& s : c->slots) {
        if (s.ev_set) (void)hipEventSynchronize(s.ev);
        for (DevBuf* b : {&s.long_list, &s.cp_bound, &s.cp_tmp, &s.cp_cursor, &s.pk_scratch, &s.pk_bound, &s.pk_tmp, &s.str_stage, &s.sd_meta,
                          &s.sd_hblob, &s.sd_stage, &s.bs_meta, &s.bs_stage, &s.bs_out, &s.ba_buf, &s.bp_hash, &s.bp_buf})
            (void)hipFree(b->p);
        if (s.ev) (void)hipEventDestroy(s.ev);
    }
    for (int j = 0; j < hpk_ctx::kMaxChunks; ++j) {
        if (c->ev_in[j]) (void)hipEventDestroy(c->ev_in[j]);
        if (c->ev_run[j]) (void)hipEventDestroy(c->ev_run[j]);
        if (c->ev_out[j]) (void)hipEventDestroy(c->ev_out[j]);
    }
    if (c->h2d) (void)hipStreamDestroy(c->h2d);
    if (c->d2h) (void)hipStreamDestroy(c->d2h);
    if (c->own) (void)hipStreamDestroy(c->own);
    delete c;
}

extern "C" int hpk_ctx_set_stream(hpk_ctx* c, void* s) {
    if (!c) return HPK_E_INVAL;
    if (s == HPK_STREAM_LEGACY)
        c->stream = (hipStream_t)0;
    else
        c->stream = s ? (hipStream_t)s : c->own;
    return HPK_E_OK;
}

extern "C" int hpk_host_register(void* ptr, size_t bytes) {
    if (!ptr || !bytes) return hpk_set_err_msg("null range", HPK_E_INVAL);
    HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    return HPK_E_OK;
}

extern "C" int hpk_host_unregister(void* ptr) {
    if (!ptr) return hpk_set_err_msg("null pointer", HPK_E_INVAL);
    HIP_TRY(hipHostUnregister(ptr));
    return HPK_E_OK;
}

// The context's page-locked host staging area (grow-only): the block-level calls build their
// Huffman batch in it so the batch's copies DMA straight from it. Growing waits for the context's
// stream (the old area may still be the source or target of its copies).
int hpk_ctx_pinned(hpk_ctx* c, size_t bytes, void** p) {
    if (bytes > c->h_pin_cap) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->d2h) HIP_TRY(hipStreamSynchronize(c->d2h));
        if (c->h_pin) (void)hipHostFree(c->h_pin);
        c->h_pin = nullptr;
        c->h_pin_cap = 0;
        const size_t cap = bytes + bytes / 4 + (1u << 20);
        HIP_TRY(hipHostMalloc(&c->h_pin, cap, hipHostMallocDefault));
        c->h_pin_cap = cap;
    }
    *p = c->h_pin;
    return HPK_E_OK;
}

extern "C" int hpk_ctx_set_decode_kernel(hpk_ctx* c, int kind) {
    if (!c || kind < HPK_DECODE_AUTO || kind > HPK_DECODE_WAVE) return hpk_set_err_msg("bad decode kernel", HPK_E_INVAL);
    c->decode_kernel = kind;
    return HPK_E_OK;
}

extern "C" int hpk_ctx_set_block_scan(hpk_ctx* c, int kind) {
    if (!c || (kind != HPK_BLOCK_SCAN_HOST && kind != HPK_BLOCK_SCAN_DEVICE)) return hpk_set_err_msg("bad block scan", HPK_E_INVAL);
    c->block_scan = kind;
    return HPK_E_OK;
}

int hpk_ctx_block_scan(const hpk_ctx* c) { return c ? c->block_scan : HPK_BLOCK_SCAN_HOST; }

extern "C" int hpk_ctx_set_block_apply(hpk_ctx* c, int kind) {
    if (!c || (kind != HPK_BLOCK_APPLY_HOST && kind != HPK_BLOCK_APPLY_DEVICE)) return hpk_set_err_msg("bad block apply", HPK_E_INVAL);
    c->block_apply = kind;
    return HPK_E_OK;
}

int hpk_ctx_block_apply(const hpk_ctx* c) { return c ? c->block_apply : HPK_BLOCK_APPLY_HOST; }

extern "C" int hpk_ctx_set_block_plan(hpk_ctx* c, int kind) {
    if (!c || (kind != HPK_BLOCK_PLAN_HOST && kind != HPK_BLOCK_PLAN_DEVICE)) return hpk_set_err_msg("bad block plan", HPK_E_INVAL);
    c->block_plan = kind;
    return HPK_E_OK;
}

int hpk_ctx_block_plan(const hpk_ctx* c) { return c ? c->block_plan : HPK_BLOCK_PLAN_HOST; }
void hpk_ctx_plan_answered(hpk_ctx* c) { c->plan_calls += 1; }
extern "C" uint64_t hpk_test_plan_calls(const hpk_ctx* c) { return c ? c->plan_calls : 0u; }

extern "C" void* hpk_ctx_stream(hpk_ctx* c) { return c ? (void*)c->stream : nullptr; }

extern "C" int hpk_ctx_set_small_mode(hpk_ctx* c, uint32_t max_literals, int workgroups, uint32_t idle_ms) {
    if (!c) return HPK_E_INVAL;
    HIP_TRY(hipSetDevice(c->device));
    if (max_literals == 0) {
        const int rc = hpk_persist_stop(c);
        c->sm_max = 0;
        return rc;
    }
    if (workgroups < 1 || workgroups > 16 || workgroups >= c->num_cu || idle_ms < 1 || idle_ms > 10000 ||
        max_literals > (uint32_t)workgroups * 256u * 64u)
        return hpk_set_err_msg("small mode: 1-16 workgroups, 1-10000 ms idle, at most 64 literals per lane", HPK_E_INVAL);
    if (!c->h_sm) {
        HIP_TRY(hipStreamCreateWithFlags(&c->sm_stream, hipStreamNonBlocking));
        HIP_TRY(hipHostMalloc(&c->h_sm, 256, hipHostMallocMapped | hipHostMallocCoherent));
        memset(c->h_sm, 0, 256);
        HIP_TRY(hipHostGetDevicePointer(&c->d_sm, c->h_sm, 0));
        HIP_TRY(hipMalloc(&c->d_sm_dev, 128));  // [0..4) counters, [4, 21) the request copy
    }
    if (c->sm_launched && (workgroups != c->sm_wgs || idle_ms != c->sm_idle_ms))
        if (int rc = hpk_persist_stop(c)) return rc;
    c->sm_max = max_literals;
    c->sm_wgs = workgroups;
    c->sm_idle_ms = idle_ms;
    return c->sm_launched ? HPK_E_OK : hpk_persist_start(c);
}

extern "C" int hpk_ctx_sync(hpk_ctx* c) {
    if (!c) return HPK_E_INVAL;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return HPK_E_OK;
}

static int check_offsets(const uint32_t* off, uint32_t n, size_t cap) {
    for (uint32_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return hpk_set_err_msg("offsets must be non-decreasing", HPK_E_INVAL);
    if (off[n] > cap || off[n] > HPK_MAX_OFFSET) return hpk_set_err_msg("offsets pass the blob's capacity", HPK_E_INVAL);
    return HPK_E_OK;
}

// read and clear the sticky device error flag (the ctx stream must be synchronised)
static int take_err(hpk_ctx* c) {
    if (!__atomic_exchange_n(c->h_err, 0u, __ATOMIC_ACQ_REL)) return HPK_E_OK;
    return hpk_set_err_msg("a batch had non-monotone offsets or offsets past a blob's capacity (HPK_BAD_OFFSETS)",
                           HPK_E_INVAL);
}

extern "C" int hpk_ctx_check(hpk_ctx* c) {
    if (!c) return HPK_E_INVAL;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return take_err(c);
}

// the end of a device-pointer call: an asynchronous one returns, a synchronous one waits and reports bad offsets
static int call_end(hpk_ctx* c, int flags) {
    if (flags & HPK_ASYNC) return HPK_E_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return take_err(c);
}

typedef int (*launch_fn)(hpk_ctx*, const hpk_batch&);

// the region form's decode as a launch_fn: the stream's slot with its list, the launch, the slot used
static int decode_region(hpk_ctx* c, const hpk_batch& b) {
    hpk_slot* s;
    int rc;
    if ((rc = slot_acquire(c, &s)) || (rc = slot_reserve(c, s, {{&s->long_list, 4 * (size_t)b.n}}))) return rc;
    if ((rc = hpk_launch_decode(c, b, s->long_list.as<uint32_t>()))) return rc;
    return slot_commit(c, s);
}

static uint32_t clamp_cap(size_t cap) { return cap > HPK_MAX_OFFSET ? HPK_MAX_OFFSET : (uint32_t)cap; }

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
    if (!trusted && (check_offsets(in_off, n, in_cap) || check_offsets(out_off, n, out_cap))) return HPK_E_INVAL;
    if (n == 0) return HPK_E_OK;
    const size_t in_bytes = in_off[n], out_bytes = out_off[n];
    if ((in_bytes && !in_blob) || (out_bytes && !out_blob)) return hpk_set_err_msg("null blob", HPK_E_INVAL);
    int rc;
    if ((rc = grow((void**)&c->d_in, &c->d_in_cap, in_bytes + 16))) return rc;
    if ((rc = grow((void**)&c->d_out, &c->d_out_cap, out_bytes + 16))) return rc;
    if ((rc = grow((void**)&c->d_meta, &c->d_meta_cap, (3 * (size_t)n + 2) * 4))) return rc;
    if ((rc = grow((void**)&c->d_st, &c->d_st_cap, n))) return rc;
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
    const size_t kChunkBytes = (size_t)4 << 20;
    int chunks = (int)((in_bytes + out_bytes) / kChunkBytes);
    chunks = chunks < 1 ? 1 : (chunks > hpk_ctx::kMaxChunks ? hpk_ctx::kMaxChunks : chunks);
    if ((uint32_t)chunks > n) chunks = (int)n;
    cut[0] = 0;
    for (int j = 1; j < chunks; ++j) {  // first literal whose end passes j/chunks of the bytes
        const uint64_t target = (uint64_t)in_bytes * j / chunks;
        uint32_t lo = cut[j - 1], hi = n;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (in_off[mid + 1] < target) lo = mid + 1; else hi = mid;
        }
        cut[j] = lo;
    }
    cut[chunks] = n;
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
    return take_err(c);
}

static int run_batch(launch_fn fn, hpk_ctx* c, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off,
                     uint32_t n, uint8_t* out_blob, size_t out_cap, const uint32_t* out_off, uint32_t* out_len,
                     uint8_t* status, int flags) {
    if (!c || !in_off || !out_off || (n && (!out_len || !status))) return hpk_set_err_msg("null argument", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    if (flags & HPK_PTR_DEVICE) {
        if (n == 0) return HPK_E_OK;
        if (!in_blob || !out_blob) return hpk_set_err_msg("null blob", HPK_E_INVAL);
        const hpk_batch b{in_blob, clamp_cap(in_cap), in_off, n, out_blob, clamp_cap(out_cap), out_off, out_len, status};
        if (fn == decode_region && !(flags & HPK_ASYNC) && c->sm_max) {  // the small-call mode
            bool handled = false;
            if (int rc = hpk_persist_call(c, b, &handled)) return rc;
            if (handled) return HPK_E_OK;
        }
        if (int rc = fn(c, b)) return rc;
        return call_end(c, flags);
    }
    int chunks;
    uint32_t cut[hpk_ctx::kMaxChunks + 1];
    if (int rc = host_begin(fn, c, in_blob, in_cap, in_off, n, out_blob, out_cap, out_off, out_len, status, false,
                            &chunks, cut))
        return rc;
    return chunks ? host_end(c) : HPK_E_OK;
}

// The block decoder's form (hpk_hpack.cpp): a trusted host batch started here, its chunks' results
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

// The argument checks that the compacted form, the packed form and the pack share; `what` names the caller in
// the messages. in_cap (the two decodes): *need = the bytes that hold every literal's 4-rounded decoded bound.
static int check_call(const hpk_ctx* c, bool null_arg, int flags, uint32_t n, const char* what, const size_t* in_cap,
                      uint64_t* need) {
    auto inval = [&](const char* before, const char* after) {
        return hpk_set_err_msg((std::string(before) + what + after).c_str(), HPK_E_INVAL);
    };
    if (!c || null_arg) return hpk_set_err_msg("null argument", HPK_E_INVAL);
    if (!(flags & HPK_PTR_DEVICE)) return inval("the ", " takes device pointers only");
    if (n >= 0x7FFFFFFFu) return inval("too many literals for the ", "");
    if (in_cap) {
        *need = (uint64_t)hpk_decoded_bound(clamp_cap(*in_cap)) + 4ull * n;
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
    if (int rc = check_call(c, !in_off || !out_off || (n && (!out_len || !status)), flags, n, "compacted form", &in_cap,
                            &need))
        return rc;
    if (out_cap < need) return hpk_set_err_msg("out_cap below hpk_decoded_bound(in_cap) + 4 n", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(out_off, 0, 4, c->stream));
        return call_end(c, flags);
    }
    if (!in_blob || !out_blob) return hpk_set_err_msg("null blob", HPK_E_INVAL);
    const bool wave = hpk_compact_wave(c, n);
    hpk_slot* s;
    int rc;
    if ((rc = slot_acquire(c, &s))) return rc;
    if (wave)
        rc = slot_reserve(c, s, {{&s->long_list, 4 * (size_t)n}});
    else
        rc = slot_reserve(c, s, {{&s->long_list, 4 * (size_t)n}, {&s->cp_bound, 4 * ((size_t)n + 1)},
                                 {&s->cp_tmp, hpk_bound_tmp_bytes(n)}, {&s->cp_cursor, 4}});
    if (rc) return rc;
    hpk_batch b{in_blob, clamp_cap(in_cap), in_off, n, out_blob, clamp_cap(out_cap), nullptr, out_len, status};
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
    if ((rc = slot_commit(c, s))) return rc;
    return call_end(c, flags);
}

// The end of a packed call: a synchronous one waits, then reports bad offsets (HPK_E_INVAL) before a
// result that did not fit (HPK_E_NOSPACE: dst_off[n] read back with the wait).
static int packed_end(hpk_ctx* c, const uint32_t* dst_off_n, size_t dst_cap, int flags) {
    if (flags & HPK_ASYNC) return HPK_E_OK;
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, dst_off_n, 4, hipMemcpyDeviceToHost, c->stream));
    if (int rc = call_end(c, flags)) return rc;
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
    if (int rc = check_call(c, !in_off || !out_off || (n && (!out_len || !status)), flags, n, "packed form", &in_cap, &need))
        return rc;
    if (n && (!in_blob || (!out_blob && out_cap))) return hpk_set_err_msg("null blob", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(out_off, 0, 4, c->stream));
        return packed_end(c, out_off, out_cap, flags);
    }
    size_t tmp = hpk_bound_tmp_bytes(n);  // (the two scans follow each other: one scratch)
    if (tmp < hpk_pack_tmp_bytes(n)) tmp = hpk_pack_tmp_bytes(n);
    hpk_slot* s;
    int rc;
    if ((rc = slot_acquire(c, &s)) ||
        (rc = slot_reserve(c, s, {{&s->long_list, 4 * (size_t)n}, {&s->pk_bound, 4 * ((size_t)n + 1)}, {&s->pk_tmp, tmp},
                                  {&s->pk_scratch, (size_t)need + 64}})))
        return rc;
    uint32_t* bound = s->pk_bound.as<uint32_t>();
    uint8_t* scratch = s->pk_scratch.as<uint8_t>();
    if ((rc = hpk_bound_scan(c, in_off, n, bound, s->pk_tmp.p))) return rc;
    const hpk_batch b{in_blob, clamp_cap(in_cap), in_off, n, scratch, (uint32_t)need, bound, out_len, status};
    if ((rc = hpk_launch_decode(c, b, s->long_list.as<uint32_t>()))) return rc;
    if ((rc = hpk_pack_launch(c, scratch, (uint32_t)need, bound, out_len, n, out_blob, clamp_cap(out_cap), out_off,
                              s->pk_tmp.p, need)))
        return rc;
    if ((rc = slot_commit(c, s))) return rc;
    return packed_end(c, out_off + n, out_cap, flags);
}

// The pack step on its own: results already held in the region or compacted layout, laid end to end.
extern "C" int hpk_pack_batch(hpk_ctx* c, const uint8_t* src_blob, size_t src_cap, const uint32_t* src_off,
                              const uint32_t* src_len, uint32_t n, uint8_t* dst_blob, size_t dst_cap, uint32_t* dst_off,
                              int flags) {
    if (int rc = check_call(c, !dst_off || (n && (!src_off || !src_len)), flags, n, "pack", nullptr, nullptr)) return rc;
    if (n && ((!src_blob && src_cap) || (!dst_blob && dst_cap))) return hpk_set_err_msg("null blob", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    hpk_slot* s;
    int rc;
    if ((rc = slot_acquire(c, &s)) || (rc = slot_reserve(c, s, {{&s->pk_tmp, hpk_pack_tmp_bytes(n)}}))) return rc;
    if ((rc = hpk_pack_launch(c, src_blob, clamp_cap(src_cap), src_off, src_len, n, dst_blob, clamp_cap(dst_cap), dst_off,
                              s->pk_tmp.p, HPK_MAX_OFFSET)))
        return rc;
    if ((rc = slot_commit(c, s))) return rc;
    return packed_end(c, dst_off + n, dst_cap, flags);
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
    if (int rc = check_call(c, !in_off || (n && !out_len), flags, n, "encoded-length call", nullptr, nullptr)) return rc;
    if (n == 0) return HPK_E_OK;
    if (!in_blob && in_cap) return hpk_set_err_msg("null blob", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    // (a blob of no bytes: the kernel's clamped loads still read one chunk, so give them one that exists)
    if (!in_blob || !in_cap) in_blob = reinterpret_cast<const uint8_t*>(c->d_codes), in_cap = 0;
    if (int rc = hpk_launch_enclen(c, in_blob, clamp_cap(in_cap), in_off, n, out_len, nullptr)) return rc;
    return call_end(c, flags);
}

// The packed encode (include/hpk.h): the length pass writes out_len and status, the length scan out_off, and
// the encode kernel's packed instantiation writes every literal at its final place, clipped at out_cap. The
// only scratch is the scan's tile sums; the word after them is the scan's verdict on the total.
extern "C" int hpk_encode_batch_packed(hpk_ctx* c, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off,
                                       uint32_t n, uint8_t* out_blob, size_t out_cap, uint32_t* out_off,
                                       uint32_t* out_len, uint8_t* status, int flags) {
    if (int rc = check_call(c, !in_off || !out_off || (n && (!out_len || !status)), flags, n, "packed encode", nullptr,
                            nullptr))
        return rc;
    if (n && ((!in_blob && in_cap) || (!out_blob && out_cap))) return hpk_set_err_msg("null blob", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(out_off, 0, 4, c->stream));
        return packed_end(c, out_off, out_cap, flags);
    }
    const size_t tmp = hpk_pack_tmp_bytes(n);
    hpk_slot* s;
    int rc;
    if ((rc = slot_acquire(c, &s)) || (rc = slot_reserve(c, s, {{&s->pk_tmp, tmp + 32}}))) return rc;
    // (blobs of no bytes: addresses that exist for the kernels' base pointers; with a capacity of 0 no byte
    // of them is written, and the input's clamped loads read one chunk of the code table)
    if (!in_blob || !in_cap) in_blob = reinterpret_cast<const uint8_t*>(c->d_codes), in_cap = 0;
    if (!out_blob || !out_cap) out_blob = s->pk_tmp.as<uint8_t>() + ((tmp + 15) & ~(size_t)15), out_cap = 0;
    if ((rc = hpk_launch_enclen(c, in_blob, clamp_cap(in_cap), in_off, n, out_len, status))) return rc;
    if ((rc = hpk_len_scan(c, out_len, n, out_off, s->pk_tmp.p))) return rc;
    const hpk_batch b{in_blob, clamp_cap(in_cap), in_off, n, out_blob, clamp_cap(out_cap), out_off, out_len, status};
    if ((rc = hpk_launch_encode_packed(c, b, hpk_len_scan_verdict(s->pk_tmp.p, n)))) return rc;
    if ((rc = slot_commit(c, s))) return rc;
    return packed_end(c, out_off + n, out_cap, flags);
}

// The string-literal lengths alone (include/hpk.h): the length pass and its form step, no scratch.
extern "C" int hpk_string_len_batch(hpk_ctx* c, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off, uint32_t n,
                                    const uint8_t* policy, uint32_t* out_len, int flags) {
    if (int rc = check_call(c, !in_off || (n && !out_len), flags, n, "string-length call", nullptr, nullptr)) return rc;
    if (n == 0) return HPK_E_OK;
    if (!in_blob && in_cap) return hpk_set_err_msg("null blob", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    if (!in_blob || !in_cap) in_blob = reinterpret_cast<const uint8_t*>(c->d_codes), in_cap = 0;
    int rc;
    if ((rc = hpk_launch_enclen(c, in_blob, clamp_cap(in_cap), in_off, n, out_len, nullptr)) ||
        (rc = hpk_launch_strlen_form(c, clamp_cap(in_cap), in_off, n, policy, out_len, nullptr)))
        return rc;
    return call_end(c, flags);
}

// The string-literal encode's steps on device arrays (s: the stream's slot, pk_tmp reserved with tmp + 32
// bytes): the length pass and its form step write out_len and status, the length scan out_off, and the emit
// kernel every representation at its final place, clipped at out_cap.
static int strings_steps(hpk_ctx* c, hpk_slot* s, size_t tmp, const uint8_t* in_blob, uint32_t in_cap,
                         const uint32_t* in_off, uint32_t n, const uint8_t* policy, uint8_t* out_blob, uint32_t out_cap,
                         uint32_t* out_off, uint32_t* out_len, uint8_t* status) {
    // (blobs of no bytes: addresses that exist, as hpk_encode_batch_packed)
    if (!in_blob || !in_cap) in_blob = reinterpret_cast<const uint8_t*>(c->d_codes), in_cap = 0;
    if (!out_blob || !out_cap) out_blob = s->pk_tmp.as<uint8_t>() + ((tmp + 15) & ~(size_t)15), out_cap = 0;
    int rc;
    if ((rc = hpk_launch_enclen(c, in_blob, in_cap, in_off, n, out_len, nullptr)) ||
        (rc = hpk_launch_strlen_form(c, in_cap, in_off, n, policy, out_len, status)) ||
        (rc = hpk_len_scan(c, out_len, n, out_off, s->pk_tmp.p)))
        return rc;
    const hpk_batch b{in_blob, in_cap, in_off, n, out_blob, out_cap, out_off, out_len, status};
    return hpk_launch_encode_strings(c, b, policy, hpk_len_scan_verdict(s->pk_tmp.p, n));
}

// The host form: offsets and policies checked before anything is copied, the input staged into the slot's
// scratch in one piece, the steps, out_off[n] read back, then exactly the bytes written and the three arrays.
static int strings_host(hpk_ctx* c, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off, uint32_t n,
                        const uint8_t* policy, uint8_t* out_blob, size_t out_cap, uint32_t* out_off, uint32_t* out_len,
                        uint8_t* status) {
    if (check_offsets(in_off, n, in_cap)) return HPK_E_INVAL;
    uint64_t bound = 0;  // no representation is longer: len + 6, or the Huffman bound + 6 where that form is forced
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t pol = policy ? policy[i] : (uint32_t)HPK_STR_AUTO, len = in_off[i + 1] - in_off[i];
        if (pol > HPK_STR_VERBATIM) return hpk_set_err_msg("string policy above HPK_STR_VERBATIM", HPK_E_INVAL);
        bound += (pol == HPK_STR_HUFFMAN ? hpk_encoded_bound(len) : (size_t)len) + 6u;
    }
    if (n == 0) {
        out_off[0] = 0;
        return HPK_E_OK;
    }
    const size_t in_bytes = in_off[n];
    const uint32_t dcap = clamp_cap(bound < out_cap ? (size_t)bound : out_cap);
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t at_ioff = up16(in_bytes + 16), at_ooff = at_ioff + up16(4 * ((size_t)n + 1));
    const size_t at_len = at_ooff + up16(4 * ((size_t)n + 1)), at_pol = at_len + up16(4 * (size_t)n);
    const size_t at_st = at_pol + up16(n), at_out = at_st + up16(n);
    const size_t tmp = hpk_pack_tmp_bytes(n);
    hpk_slot* s;
    int rc;
    if ((rc = slot_acquire(c, &s)) ||
        (rc = slot_reserve(c, s, {{&s->pk_tmp, tmp + 32}, {&s->str_stage, at_out + (size_t)dcap + 16}})))
        return rc;
    uint8_t* d = s->str_stage.as<uint8_t>();
    uint32_t* d_ioff = reinterpret_cast<uint32_t*>(d + at_ioff);
    uint32_t* d_ooff = reinterpret_cast<uint32_t*>(d + at_ooff);
    uint32_t* d_len = reinterpret_cast<uint32_t*>(d + at_len);
    if (in_bytes > in_off[0])
        HIP_TRY(hipMemcpyAsync(d + in_off[0], in_blob + in_off[0], in_bytes - in_off[0], hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_ioff, in_off, 4 * ((size_t)n + 1), hipMemcpyHostToDevice, c->stream));
    if (policy) HIP_TRY(hipMemcpyAsync(d + at_pol, policy, n, hipMemcpyHostToDevice, c->stream));
    if ((rc = strings_steps(c, s, tmp, d, (uint32_t)in_bytes, d_ioff, n, policy ? d + at_pol : nullptr, d + at_out, dcap,
                            d_ooff, d_len, d + at_st)))
        return rc;
    HIP_TRY(hipMemcpyAsync(out_off, d_ooff, 4 * ((size_t)n + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(out_len, d_len, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(status, d + at_st, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t total = out_off[n], give = total < out_cap ? total : out_cap;
    if (give) {
        HIP_TRY(hipMemcpyAsync(out_blob, d + at_out, give, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if ((rc = slot_commit(c, s)) || (rc = take_err(c))) return rc;
    if (total > out_cap) return hpk_set_err_msg("the packed bytes pass the output capacity", HPK_E_NOSPACE);
    return HPK_E_OK;
}

// The packed string-literal encode (include/hpk.h).
extern "C" int hpk_encode_strings_packed(hpk_ctx* c, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off,
                                         uint32_t n, const uint8_t* policy, uint8_t* out_blob, size_t out_cap,
                                         uint32_t* out_off, uint32_t* out_len, uint8_t* status, int flags) {
    if (!c || !in_off || !out_off || (n && (!out_len || !status))) return hpk_set_err_msg("null argument", HPK_E_INVAL);
    if (n >= 0x7FFFFFFFu) return hpk_set_err_msg("too many literals for the string-literal encode", HPK_E_INVAL);
    if (n && ((!in_blob && in_cap) || (!out_blob && out_cap))) return hpk_set_err_msg("null blob", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    if (!(flags & HPK_PTR_DEVICE))
        return strings_host(c, in_blob, in_cap, in_off, n, policy, out_blob, out_cap, out_off, out_len, status);
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(out_off, 0, 4, c->stream));
        return packed_end(c, out_off, out_cap, flags);
    }
    const size_t tmp = hpk_pack_tmp_bytes(n);
    hpk_slot* s;
    int rc;
    if ((rc = slot_acquire(c, &s)) || (rc = slot_reserve(c, s, {{&s->pk_tmp, tmp + 32}}))) return rc;
    if ((rc = strings_steps(c, s, tmp, in_blob, clamp_cap(in_cap), in_off, n, policy, out_blob, clamp_cap(out_cap),
                            out_off, out_len, status)))
        return rc;
    if ((rc = slot_commit(c, s))) return rc;
    return packed_end(c, out_off + n, out_cap, flags);
}

// The string-literal decode's scratch on one stream's slot: the parse step's arrays and the gather's offsets in
// sd_meta, the gathered Huffman blob, and what the packed decode uses (region scratch, bound layout, scans, list).
struct strdec_scratch {
    uint32_t *start, *hlen, *rlen, *hoff;
    uint8_t *pst, *sel, *hblob;
};

// (stage: the bytes of the host form's staging buffer, 0 for device pointers)
static int strdec_reserve(hpk_ctx* c, hpk_slot* s, uint32_t in_cap, uint32_t n, uint64_t need, size_t stage, strdec_scratch* k) {
    size_t tmp = hpk_bound_tmp_bytes(n);  // (the scans follow each other: one scratch)
    if (tmp < hpk_pack_tmp_bytes(n)) tmp = hpk_pack_tmp_bytes(n);
    const size_t words = 4 * (size_t)n + 4;
    if (int rc = slot_reserve(c, s, {{&s->long_list, 4 * (size_t)n}, {&s->pk_bound, 4 * ((size_t)n + 1)}, {&s->pk_tmp, tmp},
                                     {&s->pk_scratch, (size_t)need + 64}, {&s->sd_meta, 4 * words + 2 * (size_t)n + 16},
                                     {&s->sd_hblob, (size_t)in_cap + 64}, {&s->sd_stage, stage}}))
        return rc;
    uint32_t* m = s->sd_meta.as<uint32_t>();
    k->start = m;
    k->hlen = m + n;
    k->rlen = m + 2 * (size_t)n;
    k->hoff = m + 3 * (size_t)n;  // n + 1 entries
    k->pst = reinterpret_cast<uint8_t*>(m + words);
    k->sel = k->pst + n;
    k->hblob = s->sd_hblob.as<uint8_t>();
    return HPK_E_OK;
}

// The string-literal decode's steps on device arrays (hpk_decode_strings.hip has the list), s the stream's slot,
// reserved by strdec_reserve. need: hpk_decoded_bound(in_cap) + 4 n, the region scratch's bytes.
static int strdec_steps(hpk_ctx* c, hpk_slot* s, const strdec_scratch& k, uint64_t need, const uint8_t* in_blob,
                        uint32_t in_cap, const uint32_t* str_off, const uint32_t* str_end, uint32_t n, uint8_t* out_blob,
                        uint32_t out_cap, uint32_t* out_off, uint32_t* out_len, uint32_t* consumed, uint8_t* status) {
    // (blobs of no bytes: addresses that exist for the kernels' base pointers; no byte of them is read or written)
    if (!in_blob || !in_cap) in_blob = k.hblob, in_cap = 0;
    if (!out_blob || !out_cap) out_blob = k.hblob, out_cap = 0;
    uint8_t* region = s->pk_scratch.as<uint8_t>();
    uint32_t* bound = s->pk_bound.as<uint32_t>();
    int rc;
    if ((rc = hpk_launch_strparse(c, in_blob, in_cap, str_off, str_end, n, k.start, k.hlen, k.rlen, k.pst, consumed)) ||
        // the Huffman payloads end to end (the total passes in_cap only when payloads overlap: the gather then
        // stops at in_cap, the decode meets offsets past its blob and the merge voids what was cut)
        (rc = hpk_pack_launch(c, in_blob, in_cap, k.start, k.hlen, n, k.hblob, in_cap, k.hoff, s->pk_tmp.p, in_cap)) ||
        (rc = hpk_bound_scan(c, k.hoff, n, bound, s->pk_tmp.p)))
        return rc;
    const hpk_batch b{k.hblob, in_cap, k.hoff, n, region, (uint32_t)need, bound, out_len, status};
    if ((rc = hpk_launch_decode(c, b, s->long_list.as<uint32_t>())) ||
        (rc = hpk_launch_strmerge(c, n, k.start, k.hlen, k.rlen, k.pst, k.hoff, bound, (uint32_t)need, out_len, status, k.sel)) ||
        (rc = hpk_len_scan(c, out_len, n, out_off, s->pk_tmp.p)))
        return rc;
    return hpk_pack2_launch(c, region, (uint32_t)need, in_blob, in_cap, k.start, k.sel, n, out_blob, out_cap, out_off,
                            HPK_MAX_OFFSET);
}

// The host form: windows checked before anything is copied, the input staged in one piece (the bytes from the
// lowest window start to the highest window end) into the slot's scratch, the steps, out_off[n] read back, then
// exactly the bytes written and the arrays.
static int strdec_host(hpk_ctx* c, const uint8_t* in_blob, size_t in_cap, const uint32_t* str_off, const uint32_t* str_end,
                       uint32_t n, uint8_t* out_blob, size_t out_cap, uint32_t* out_off, uint32_t* out_len,
                       uint32_t* consumed, uint8_t* status) {
    const bool mirror = !str_end;
    const uint32_t* end = mirror ? str_off + 1 : str_end;
    uint64_t bound = 0;  // no string decodes to more than hpk_decoded_bound of its window
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (str_off[i] > end[i]) return hpk_set_err_msg("a string's window ends before it starts", HPK_E_INVAL);
        if (end[i] > in_cap || end[i] > HPK_MAX_OFFSET) return hpk_set_err_msg("a string's window passes the blob's capacity", HPK_E_INVAL);
        bound += hpk_decoded_bound(end[i] - str_off[i]);
        lo = str_off[i] < lo ? str_off[i] : lo;
        hi = end[i] > hi ? end[i] : hi;
    }
    if (n == 0) {
        out_off[0] = 0;
        return HPK_E_OK;
    }
    const uint32_t dev_in = hi;  // the staged blob's capacity (offsets stay absolute; nothing below lo is read)
    const uint64_t need = (uint64_t)hpk_decoded_bound(dev_in) + 4ull * n;
    if (need > HPK_MAX_OFFSET) return hpk_set_err_msg("the string-literal decode's output would pass 4 GiB", HPK_E_INVAL);
    const uint32_t dcap = clamp_cap(bound < out_cap ? (size_t)bound : out_cap);
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t at_off = up16((size_t)dev_in + 16), at_end = at_off + up16(4 * ((size_t)n + 1));
    const size_t at_ooff = at_end + up16(4 * (size_t)n), at_len = at_ooff + up16(4 * ((size_t)n + 1));
    const size_t at_con = at_len + up16(4 * (size_t)n), at_st = at_con + up16(4 * (size_t)n), at_out = at_st + up16(n);
    hpk_slot* s;
    strdec_scratch k;
    int rc;
    if ((rc = slot_acquire(c, &s)) || (rc = strdec_reserve(c, s, dev_in, n, need, at_out + (size_t)dcap + 16, &k))) return rc;
    uint8_t* d = s->sd_stage.as<uint8_t>();
    uint32_t* d_off = reinterpret_cast<uint32_t*>(d + at_off);
    uint32_t* d_end = mirror ? d_off + 1 : reinterpret_cast<uint32_t*>(d + at_end);
    uint32_t* d_ooff = reinterpret_cast<uint32_t*>(d + at_ooff);
    uint32_t* d_len = reinterpret_cast<uint32_t*>(d + at_len);
    uint32_t* d_con = reinterpret_cast<uint32_t*>(d + at_con);
    if (hi > lo) HIP_TRY(hipMemcpyAsync(d + lo, in_blob + lo, hi - lo, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_off, str_off, 4 * ((size_t)n + (mirror ? 1 : 0)), hipMemcpyHostToDevice, c->stream));
    if (!mirror) HIP_TRY(hipMemcpyAsync(d_end, str_end, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    if ((rc = strdec_steps(c, s, k, need, d, dev_in, d_off, d_end, n, d + at_out, dcap, d_ooff, d_len, d_con, d + at_st)))
        return rc;
    HIP_TRY(hipMemcpyAsync(out_off, d_ooff, 4 * ((size_t)n + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(out_len, d_len, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    if (consumed) HIP_TRY(hipMemcpyAsync(consumed, d_con, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(status, d + at_st, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t total = out_off[n], give = total < out_cap ? total : out_cap;
    if (give) {
        HIP_TRY(hipMemcpyAsync(out_blob, d + at_out, give, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if ((rc = slot_commit(c, s)) || (rc = take_err(c))) return rc;
    if (total > out_cap) return hpk_set_err_msg("the packed bytes pass the output capacity", HPK_E_NOSPACE);
    return HPK_E_OK;
}

// The packed string-literal decode (include/hpk.h).
extern "C" int hpk_decode_strings_packed(hpk_ctx* c, const uint8_t* in_blob, size_t in_cap, const uint32_t* str_off,
                                         const uint32_t* str_end, uint32_t n, uint8_t* out_blob, size_t out_cap,
                                         uint32_t* out_off, uint32_t* out_len, uint32_t* consumed, uint8_t* status, int flags) {
    if (!c || !out_off || (n && (!str_off || !out_len || !status))) return hpk_set_err_msg("null argument", HPK_E_INVAL);
    if (n >= 0x7FFFFFFFu) return hpk_set_err_msg("too many strings for the string-literal decode", HPK_E_INVAL);
    if (n && ((!in_blob && in_cap) || (!out_blob && out_cap))) return hpk_set_err_msg("null blob", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    if (!(flags & HPK_PTR_DEVICE))
        return strdec_host(c, in_blob, in_cap, str_off, str_end, n, out_blob, out_cap, out_off, out_len, consumed, status);
    const uint64_t need = (uint64_t)hpk_decoded_bound(clamp_cap(in_cap)) + 4ull * n;
    if (need > HPK_MAX_OFFSET) return hpk_set_err_msg("the string-literal decode's output would pass 4 GiB", HPK_E_INVAL);
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(out_off, 0, 4, c->stream));
        return packed_end(c, out_off, out_cap, flags);
    }
    hpk_slot* s;
    strdec_scratch k;
    int rc;
    if ((rc = slot_acquire(c, &s)) || (rc = strdec_reserve(c, s, clamp_cap(in_cap), n, need, 0, &k))) return rc;
    if ((rc = strdec_steps(c, s, k, need, in_blob, clamp_cap(in_cap), str_off, str_end ? str_end : str_off + 1, n, out_blob,
                           clamp_cap(out_cap), out_off, out_len, consumed, status)))
        return rc;
    if ((rc = slot_commit(c, s))) return rc;
    return packed_end(c, out_off + n, out_cap, flags);
}

// The header-block scan's steps on device arrays (hpk_blkscan.hip has the list), s the stream's slot with
// bs_meta (8 bytes per block) and pk_tmp (hpk_pack_tmp_bytes(nblocks)) reserved: the count pass and the two scans.
// The emit pass is the caller's (the block decoder sizes its outputs by the totals before it emits).
static int blkscan_counts(hpk_ctx* c, hpk_slot* s, const uint8_t* blocks, uint32_t cap, const uint32_t* block_off,
                          uint32_t nblocks, uint32_t* field_off, uint32_t* str_blk_off, uint8_t* status) {
    uint32_t* nf = s->bs_meta.as<uint32_t>();
    uint32_t* ns = nf + nblocks;
    int rc;
    if ((rc = hpk_launch_blkcount(c, blocks, cap, block_off, nblocks, nf, ns, status)) ||
        (rc = hpk_len_scan(c, nf, nblocks, field_off, s->pk_tmp.p)) ||
        (rc = hpk_len_scan(c, ns, nblocks, str_blk_off, s->pk_tmp.p)))
        return rc;
    return HPK_E_OK;
}

static uint32_t clamp_u32(size_t x) { return x > 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)x; }

// The end of a scan call: a synchronous one reads both totals back with the wait, then reports bad offsets
// (HPK_E_INVAL) before a list that did not fit (HPK_E_NOSPACE).
static int blkscan_end(hpk_ctx* c, const uint32_t* field_off_n, size_t fields_cap, const uint32_t* str_blk_off_n,
                       size_t strs_cap, int flags) {
    if (flags & HPK_ASYNC) return HPK_E_OK;
    uint32_t tot[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&tot[0], field_off_n, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&tot[1], str_blk_off_n, 4, hipMemcpyDeviceToHost, c->stream));
    if (int rc = call_end(c, flags)) return rc;
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
    if (check_offsets(block_off, nblocks, cap)) return HPK_E_INVAL;
    if (nblocks == 0) {
        field_off[0] = 0;
        str_blk_off[0] = 0;
        return HPK_E_OK;
    }
    const uint32_t lo = block_off[0], hi = block_off[nblocks];
    const uint32_t fcap = clamp_u32(fields_cap < hi - lo ? fields_cap : hi - lo);  // (a field and a string take an
    const uint32_t scap = clamp_u32(strs_cap < hi - lo ? strs_cap : hi - lo);      // octet or more each)
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t offs = up16(4 * ((size_t)nblocks + 1));
    const size_t at_boff = up16((size_t)hi + 16), at_foff = at_boff + offs, at_soff = at_foff + offs;
    const size_t at_st = at_soff + offs, at_fields = at_st + up16(nblocks);
    const size_t at_so = at_fields + 16 * (size_t)fcap, at_se = at_so + up16(4 * (size_t)scap);
    const size_t bytes = at_se + up16(4 * (size_t)scap) + 16;
    hpk_slot* s;
    int rc;
    if ((rc = slot_acquire(c, &s)) ||
        (rc = slot_reserve(c, s, {{&s->bs_meta, 8 * (size_t)nblocks}, {&s->pk_tmp, hpk_pack_tmp_bytes(nblocks)}, {&s->bs_stage, bytes}})))
        return rc;
    uint8_t* d = s->bs_stage.as<uint8_t>();
    uint32_t* d_boff = reinterpret_cast<uint32_t*>(d + at_boff);
    uint32_t* d_foff = reinterpret_cast<uint32_t*>(d + at_foff);
    uint32_t* d_soff = reinterpret_cast<uint32_t*>(d + at_soff);
    hpk_field* d_fields = reinterpret_cast<hpk_field*>(d + at_fields);
    uint32_t* d_so = reinterpret_cast<uint32_t*>(d + at_so);
    uint32_t* d_se = reinterpret_cast<uint32_t*>(d + at_se);
    if (hi > lo) HIP_TRY(hipMemcpyAsync(d + lo, blocks + lo, hi - lo, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_boff, block_off, 4 * ((size_t)nblocks + 1), hipMemcpyHostToDevice, c->stream));
    if ((rc = blkscan_counts(c, s, d, hi, d_boff, nblocks, d_foff, d_soff, d + at_st)) ||
        (rc = hpk_launch_blkemit(c, d, hi, d_boff, nblocks, d_foff, d_soff, d_fields, fcap, d_so, d_se, scap)))
        return rc;
    HIP_TRY(hipMemcpyAsync(field_off, d_foff, 4 * ((size_t)nblocks + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(str_blk_off, d_soff, 4 * ((size_t)nblocks + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(status, d + at_st, nblocks, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t nf = field_off[nblocks], ns = str_blk_off[nblocks];
    const size_t gf = nf < fcap ? nf : fcap, gs = ns < scap ? ns : scap;
    if (gf) HIP_TRY(hipMemcpyAsync(fields, d_fields, 16 * gf, hipMemcpyDeviceToHost, c->stream));
    if (gs) {
        HIP_TRY(hipMemcpyAsync(str_off, d_so, 4 * gs, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(str_end, d_se, 4 * gs, hipMemcpyDeviceToHost, c->stream));
    }
    if (gf || gs) HIP_TRY(hipStreamSynchronize(c->stream));
    if ((rc = slot_commit(c, s)) || (rc = take_err(c))) return rc;
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
    if ((rc = slot_acquire(c, &s)) ||
        (rc = slot_reserve(c, s, {{&s->bs_meta, 8 * (size_t)nblocks + 16}, {&s->pk_tmp, hpk_pack_tmp_bytes(nblocks)}})))
        return rc;
    // (a blob or a list of no capacity: an address that exists for the kernels' base pointers; nothing of it is touched)
    if (!blocks || !cap) blocks = s->bs_meta.as<uint8_t>(), cap = 0;
    if (!fields_cap) fields = reinterpret_cast<hpk_field*>(s->bs_meta.p);
    if (!strs_cap) str_off = str_end = s->bs_meta.as<uint32_t>();
    if ((rc = blkscan_counts(c, s, blocks, (uint32_t)cap, block_off, nblocks, field_off, str_blk_off, status)) ||
        (rc = hpk_launch_blkemit(c, blocks, (uint32_t)cap, block_off, nblocks, field_off, str_blk_off, fields,
                                 clamp_u32(fields_cap), str_off, str_end, clamp_u32(strs_cap))))
        return rc;
    if ((rc = slot_commit(c, s))) return rc;
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
    if (ndecs == 0 || nblocks == 0) return call_end(c, flags);
    if (!field_off || !dec_blk_off || !dec_blk || !tabs || (headers_cap && (!fields || !headers)) || (tab_ent_cap && !tab_ent) ||
        (nstrs && (!str_out_off || !str_out_len || !str_status)))
        return hpk_set_err_msg("null array", HPK_E_INVAL);
    if (int rc = apply_static(c)) return rc;
    if (int rc = hpk_launch_blkapply(c, fields, field_off, nblocks, str_out_off, str_out_len, str_status, nstrs, str_base, static_base,
                                     dec_blk_off, dec_blk, ndecs, tabs, tab_ent, tab_ent_cap, headers, clamp_u32(headers_cap),
                                     results, c->d_static))
        return rc;
    if (flags & HPK_ASYNC) return HPK_E_OK;
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, field_off + nblocks, 4, hipMemcpyDeviceToHost, c->stream));
    if (int rc = call_end(c, flags)) return rc;
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
    if (!hdrs_cap && !plan) return call_end(c, flags);
    int rc;
    if (plan && (rc = apply_static(c))) return rc;
    hpk_slot* s = nullptr;
    if ((rc = slot_acquire(c, &s)) || (rc = slot_reserve(c, s, {{&s->bp_hash, 8 * hdrs_cap + 8}}))) return rc;
    if ((rc = hpk_launch_blkplan(c, arena, (uint32_t)arena_cap, static_base, fields_base, prefix_base, field_off, hdr_off, nblocks,
                                 (uint32_t)hdrs_cap, enc_blk_off, enc_blk, enc_flags, plan ? nencs : 0u, tabs, tab_ent, tab_ent_cap, reps,
                                 item_off, item_len, item_policy, s->bp_hash.p, c->d_static)))
        return rc;
    if ((rc = slot_commit(c, s))) return rc;
    return call_end(c, flags);
}

// The block encoder's device-plan path (hpk_hpack.cpp, HPK_BLOCK_PLAN_DEVICE; not in the C ABI): the caller has
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
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto lap = [&](std::chrono::steady_clock::time_point* t, long* us) {
        if (timing) (void)hipStreamSynchronize(c->stream);
        const auto t1 = now();
        *us = (long)std::chrono::duration_cast<std::chrono::microseconds>(t1 - *t).count();
        *t = t1;
    };
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t at_foff = up16(arena_cap + 16), at_hoff = at_foff + up16(4 * (2 * (size_t)nh + 1));
    const size_t at_eoff = at_hoff + up16(4 * ((size_t)nb + 1)), at_eblk = at_eoff + up16(4 * ((size_t)ne + 1));
    const size_t at_flag = at_eblk + up16(4 * (size_t)nb), at_tabs = at_flag + up16(ne);
    const size_t at_ent = at_tabs + up16(32 * (size_t)ne), at_reps = at_ent + up16(16 * (size_t)job->nent);
    const size_t at_ioff = at_reps + 16 * (size_t)nh, at_ilen = at_ioff + up16(4 * (size_t)ni), at_ipol = at_ilen + up16(4 * (size_t)ni);
    const size_t at_in = at_ipol + up16(ni), at_inoff = at_in + up16(in_cap + 16);
    const size_t at_ooff = at_inoff + up16(4 * ((size_t)ni + 1)), at_olen = at_ooff + up16(4 * ((size_t)ni + 1));
    const size_t at_st = at_olen + up16(4 * (size_t)ni), at_boff = at_st + up16(ni), at_out = at_boff + up16(4 * ((size_t)nb + 1));
    const size_t tmp = hpk_pack_tmp_bytes(ni);
    hpk_slot* s;
    int rc;
    if ((rc = apply_static(c)) || (rc = slot_acquire(c, &s)) ||
        (rc = slot_reserve(c, s, {{&s->bp_hash, 8 * (size_t)nh + 8}, {&s->pk_tmp, tmp + 32}, {&s->bp_buf, at_out + out_cap + 16}})))
        return rc;
    auto t0 = now();
    uint8_t* d = s->bp_buf.as<uint8_t>();
    auto u32p = [&](size_t at) { return reinterpret_cast<uint32_t*>(d + at); };
    auto up = [&](size_t at, const void* src, size_t bytes) {
        return bytes ? hipMemcpyAsync(d + at, src, bytes, hipMemcpyHostToDevice, c->stream) : hipSuccess;
    };
    HIP_TRY(up(0, job->arena, job->prefix_base));
    HIP_TRY(up(at_foff, job->field_off, 4 * (2 * (size_t)nh + 1)));
    HIP_TRY(up(at_hoff, job->hdr_off, 4 * ((size_t)nb + 1)));
    HIP_TRY(up(at_eoff, job->enc_blk_off, 4 * ((size_t)ne + 1)));
    HIP_TRY(up(at_eblk, job->enc_blk, 4 * (size_t)job->enc_blk_off[ne]));
    HIP_TRY(up(at_flag, job->enc_flags, ne));
    HIP_TRY(up(at_tabs, job->tabs, 32 * (size_t)ne));
    HIP_TRY(up(at_ent, job->tab_ent, 16 * (size_t)job->nent));
    lap(&t0, &job->us_up);
    hpk_dtab* d_tabs = reinterpret_cast<hpk_dtab*>(d + at_tabs);
    hpk_header* d_ent = reinterpret_cast<hpk_header*>(d + at_ent);
    if ((rc = hpk_launch_blkplan(c, d, (uint32_t)arena_cap, 0u, job->fields_base, job->prefix_base, u32p(at_foff), u32p(at_hoff), nb, nh,
                                 u32p(at_eoff), u32p(at_eblk), d + at_flag, ne, d_tabs, d_ent, job->nent,
                                 reinterpret_cast<hpk_hrep*>(d + at_reps), u32p(at_ioff), u32p(at_ilen), d + at_ipol, s->bp_hash.p,
                                 c->d_static)))
        return rc;
    lap(&t0, &job->us_plan);
    if ((rc = hpk_pack_launch(c, d, (uint32_t)arena_cap, u32p(at_ioff), u32p(at_ilen), ni, d + at_in, (uint32_t)in_cap, u32p(at_inoff),
                              s->pk_tmp.p, in_cap)))
        return rc;
    lap(&t0, &job->us_items);
    if ((rc = strings_steps(c, s, tmp, d + at_in, (uint32_t)in_cap, u32p(at_inoff), ni, d + at_ipol, d + at_out, (uint32_t)out_cap,
                            u32p(at_ooff), u32p(at_olen), d + at_st)) ||
        (rc = hpk_launch_blkplan_boff(c, u32p(at_ooff), u32p(at_hoff), nb, u32p(at_boff))))
        return rc;
    lap(&t0, &job->us_strings);
    HIP_TRY(hipMemcpyAsync(job->tabs, d_tabs, 32 * (size_t)ne, hipMemcpyDeviceToHost, c->stream));
    if (job->nent) HIP_TRY(hipMemcpyAsync(job->tab_ent, d_ent, 16 * (size_t)job->nent, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(job->block_off, d + at_boff, 4 * ((size_t)nb + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t total = job->block_off[nb];
    uint8_t* bytes = static_cast<uint8_t*>(malloc(total ? total : 1));
    if (!bytes) return hpk_set_err_msg("out of memory", HPK_E_INVAL);
    hipError_t e = total > out_cap ? hipErrorInvalidValue : hipSuccess;
    if (e == hipSuccess && total) e = hipMemcpyAsync(bytes, d + at_out, total, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        free(bytes);
        return hpk_set_err("the planned blocks' bytes", e);
    }
    if ((rc = slot_commit(c, s)) || (rc = take_err(c))) {
        free(bytes);
        return rc;
    }
    lap(&t0, &job->us_back);
    job->bytes = bytes;
    return HPK_E_OK;
}

// The block decoder's device-scan path (hpk_hpack.cpp, HPK_BLOCK_SCAN_DEVICE; not in the C ABI): block_off is
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
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto us = [&](std::chrono::steady_clock::time_point a) {
        return (long)std::chrono::duration_cast<std::chrono::microseconds>(now() - a).count();
    };
    const auto t_0 = now();
    auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t offs = up16(4 * ((size_t)nblocks + 1));
    const size_t at_boff = up16((size_t)hi + 16), at_foff = at_boff + offs, at_soff = at_foff + offs, at_st = at_soff + offs;
    hpk_slot* s;
    int rc;
    if ((rc = slot_acquire(c, &s)) ||
        (rc = slot_reserve(c, s, {{&s->bs_meta, 8 * (size_t)nblocks}, {&s->pk_tmp, hpk_pack_tmp_bytes(nblocks)},
                                  {&s->bs_stage, at_st + up16(nblocks) + 16}})))
        return rc;
    uint8_t* d = s->bs_stage.as<uint8_t>();
    uint32_t* d_boff = reinterpret_cast<uint32_t*>(d + at_boff);
    uint32_t* d_foff = reinterpret_cast<uint32_t*>(d + at_foff);
    uint32_t* d_soff = reinterpret_cast<uint32_t*>(d + at_soff);
    if (hi > lo) HIP_TRY(hipMemcpyAsync(d + lo, blocks + lo, hi - lo, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_boff, block_off, 4 * ((size_t)nblocks + 1), hipMemcpyHostToDevice, c->stream));
    if ((rc = blkscan_counts(c, s, d, hi, d_boff, nblocks, d_foff, d_soff, d + at_st))) return rc;
    uint32_t tot[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&tot[0], d_foff + nblocks, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&tot[1], d_soff + nblocks, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint32_t nf = tot[0], ns = tot[1];
    o->us_scan = us(t_0);
    const auto t_1 = now();
    // the outputs, sized by the totals; the strings decode to no more than the blocks' decoded bound
    const uint64_t need = (uint64_t)hpk_decoded_bound(hi) + 4ull * ns;
    if (need > HPK_MAX_OFFSET) return hpk_set_err_msg("the blocks' strings would pass 4 GiB", HPK_E_INVAL);
    const uint32_t dcap = (uint32_t)hpk_decoded_bound(hi) + 16u;
    const size_t sw = up16(4 * ((size_t)ns + 1));
    const size_t at_so = 16 * (size_t)nf, at_se = at_so + sw, at_oo = at_se + sw, at_ol = at_oo + sw, at_ss = at_ol + sw;
    const size_t at_out = at_ss + up16(ns);
    strdec_scratch k{};
    if ((rc = slot_reserve(c, s, {{&s->bs_out, at_out + dcap + 16}}))) return rc;
    if (ns && (rc = strdec_reserve(c, s, hi, ns, need, 0, &k))) return rc;
    uint8_t* q = s->bs_out.as<uint8_t>();
    hpk_field* d_fields = reinterpret_cast<hpk_field*>(q);
    uint32_t* d_so = reinterpret_cast<uint32_t*>(q + at_so);
    uint32_t* d_se = reinterpret_cast<uint32_t*>(q + at_se);
    uint32_t* d_oo = reinterpret_cast<uint32_t*>(q + at_oo);
    uint32_t* d_ol = reinterpret_cast<uint32_t*>(q + at_ol);
    if ((rc = hpk_launch_blkemit(c, d, hi, d_boff, nblocks, d_foff, d_soff, d_fields, nf, d_so, d_se, ns))) return rc;
    if (ns && (rc = strdec_steps(c, s, k, need, d, hi, d_so, d_se, ns, q + at_out, dcap, d_oo, d_ol, nullptr, q + at_ss)))
        return rc;
    // back into the page-locked area: fields | field_off | out_off | out_len | status | the packed bytes
    const size_t h_foff = 16 * (size_t)nf, h_oo = h_foff + offs, h_ol = h_oo + sw, h_ss = h_ol + sw, h_out = h_ss + up16(ns);
    // (with a plan, behind them: results | tabs | headers | the tables' entries)
    const size_t nd = plan ? plan->ndecs : 0, ne = plan ? plan->nent : 0;
    const size_t h_res = up16(h_out + dcap + 16), h_tabs = h_res + 16 * (size_t)nblocks, h_hdr = h_tabs + 32 * nd;
    const size_t h_ent = h_hdr + 16 * (size_t)nf;
    uint8_t* h = nullptr;
    if ((rc = hpk_ctx_pinned(c, plan ? h_ent + 16 * ne + 16 : h_out + dcap + 16, (void**)&h))) return rc;
    if (plan) {
        // HPK_BLOCK_APPLY_DEVICE: the lists and the tables go up, hpk_apply_blocks' kernel runs on what the steps
        // above left on the device, and the results, the tables' records and the strings' total come back. Nothing
        // deferred: the header records, the tables' entries and exactly the packed bytes follow, and the field
        // records and the strings' arrays stay where they are. Else the call goes on as without a plan.
        const auto t_a = now();
        plan->applied = 0;
        const size_t a_off = up16(4 * (nd + 1)), a_blk = up16(4 * (size_t)nblocks);
        const size_t at_blk = a_off, at_tabs = at_blk + a_blk, at_ent = at_tabs + 32 * nd, at_res = at_ent + 16 * ne;
        const size_t at_hdr = at_res + 16 * (size_t)nblocks;
        if ((rc = slot_reserve(c, s, {{&s->ba_buf, at_hdr + 16 * (size_t)nf + 16}})) || (rc = apply_static(c))) return rc;
        uint8_t* a = s->ba_buf.as<uint8_t>();
        HIP_TRY(hipMemcpyAsync(a, plan->dec_blk_off, 4 * (nd + 1), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(a + at_blk, plan->dec_blk, 4 * (size_t)nblocks, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(a + at_tabs, plan->tabs, 32 * nd, hipMemcpyHostToDevice, c->stream));
        if (ne) HIP_TRY(hipMemcpyAsync(a + at_ent, plan->tab_ent, 16 * ne, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemsetAsync(a + at_res, 0, 16 * ((size_t)nblocks + nf), c->stream));  // the results and the header records
        if ((rc = hpk_launch_blkapply(c, d_fields, d_foff, nblocks, d_oo, d_ol, q + at_ss, ns, plan->str_base, 0u,
                                      reinterpret_cast<uint32_t*>(a), reinterpret_cast<uint32_t*>(a + at_blk), plan->ndecs,
                                      reinterpret_cast<hpk_dtab*>(a + at_tabs), reinterpret_cast<hpk_header*>(a + at_ent), ne,
                                      reinterpret_cast<hpk_header*>(a + at_hdr), nf,
                                      reinterpret_cast<hpk_block_result*>(a + at_res), c->d_static)))
            return rc;
        uint32_t total = 0;
        HIP_TRY(hipMemcpyAsync(h + h_res, a + at_res, 16 * (size_t)nblocks, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(h + h_tabs, a + at_tabs, 32 * nd, hipMemcpyDeviceToHost, c->stream));
        if (ns) HIP_TRY(hipMemcpyAsync(&total, d_oo + ns, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if ((rc = take_err(c))) return rc;  // (a void decoder: the lists or the tables the host made are wrong)
        const hpk_dtab* tb = reinterpret_cast<const hpk_dtab*>(h + h_tabs);
        bool deferred = false;
        for (size_t k = 0; k < nd; ++k) deferred |= tb[k].applied != plan->dec_blk_off[k + 1] - plan->dec_blk_off[k];
        plan->us_apply = us(t_a);
        if (!deferred) {
            if (total > dcap) return hpk_set_err_msg("the blocks' strings pass their decoded bound", HPK_E_DEVICE);
            if (nf) HIP_TRY(hipMemcpyAsync(h + h_hdr, a + at_hdr, 16 * (size_t)nf, hipMemcpyDeviceToHost, c->stream));
            if (ne) HIP_TRY(hipMemcpyAsync(h + h_ent, a + at_ent, 16 * ne, hipMemcpyDeviceToHost, c->stream));
            if (total) HIP_TRY(hipMemcpyAsync(h + h_out, q + at_out, total, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            if ((rc = slot_commit(c, s))) return rc;
            plan->applied = 1;
            plan->results = reinterpret_cast<const hpk_block_result*>(h + h_res);
            plan->tabs_out = tb;
            plan->headers = reinterpret_cast<const hpk_header*>(h + h_hdr);
            plan->ent_out = reinterpret_cast<const hpk_header*>(h + h_ent);
            plan->packed_len = total;
            o->arena = h + h_out;
            o->nfields = nf;
            o->nstrs = ns;
            o->us_strings = us(t_1);
            return HPK_E_OK;
        }
    }
    if (nf) HIP_TRY(hipMemcpyAsync(h, d_fields, 16 * (size_t)nf, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(h + h_foff, d_foff, 4 * ((size_t)nblocks + 1), hipMemcpyDeviceToHost, c->stream));
    uint32_t* h_off = reinterpret_cast<uint32_t*>(h + h_oo);
    h_off[0] = 0;
    if (ns) {
        HIP_TRY(hipMemcpyAsync(h_off, d_oo, 4 * ((size_t)ns + 1), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(h + h_ol, d_ol, 4 * (size_t)ns, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(h + h_ss, q + at_ss, ns, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    o->us_strings = us(t_1);
    const auto t_2 = now();
    const uint32_t total = h_off[ns];
    if (total > dcap) return hpk_set_err_msg("the blocks' strings pass their decoded bound", HPK_E_DEVICE);
    if (total) {
        HIP_TRY(hipMemcpyAsync(h + h_out, q + at_out, total, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if ((rc = slot_commit(c, s))) return rc;
    o->fields = reinterpret_cast<const hpk_field*>(h);
    o->field_off = reinterpret_cast<const uint32_t*>(h + h_foff);
    o->out_off = h_off;
    o->out_len = reinterpret_cast<const uint32_t*>(h + h_ol);
    o->status = h + h_ss;
    o->arena = h + h_out;
    o->nfields = nf;
    o->nstrs = ns;
    o->us_back = us(t_2);
    return HPK_E_OK;
}

// buffet's buffer arena (crates/buffet/src/bufpool/privatepool.rs:80-108): ONE anonymous mapping of
// num_bufs x buf_size bytes from which a thread's read buffers are carved; page-locked here (pin) so
// batches whose literal or frame bytes sit in it DMA without a staging copy.
struct hpk_arena {
    void* base;
    size_t len;
    int pinned;
};

extern "C" hpk_arena* hpk_arena_create(size_t num_bufs, size_t buf_size, int pin) {
    if (!num_bufs || !buf_size || num_bufs > ((size_t)1 << 40) / buf_size) {
        hpk_set_err_msg("bad arena size", HPK_E_INVAL);
        return nullptr;
    }
    const size_t len = num_bufs * buf_size;
    void* p = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (p == MAP_FAILED) {
        hpk_set_err_msg("mmap failed", HPK_E_INVAL);
        return nullptr;
    }
    hpk_arena* a = new hpk_arena{p, len, 0};
    if (pin) {
        const hipError_t e = hipHostRegister(p, len, hipHostRegisterDefault);
        if (e != hipSuccess) {
            hpk_set_err("hipHostRegister arena", e);
            munmap(p, len);
            delete a;
            return nullptr;
        }
        a->pinned = 1;
    }
    return a;
}

extern "C" void* hpk_arena_base(const hpk_arena* a) { return a ? a->base : nullptr; }
extern "C" size_t hpk_arena_len(const hpk_arena* a) { return a ? a->len : 0; }

extern "C" void hpk_arena_destroy(hpk_arena* a) {
    if (!a) return;
    if (a->pinned) (void)hipHostUnregister(a->base);
    munmap(a->base, a->len);
    delete a;
}
