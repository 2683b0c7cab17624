// hpk_ctx.hip — the device context of the C ABI (include/hpk.h) and its per-stream slots. The batch entry points
// are in hpk_calls_batch.hip, hpk_calls_strings.hip, hpk_calls_blocks.hip and hpk_calls_frames.hip.
#include <stdio.h>
#include <string.h>
#include <sys/mman.h>

#include "hpk_calls.h"

#define HPK_VERSION "hpk 0.48 gfx950 decode v42 (every batch: wave fills, each wave with its own LDS window and image, lookups in a 13-bit two-symbol table, the lane loop in rounds of four nested body steps with long codes taken once a round, longest-first queue sorted under the previous image's LDS read-out, the next fill's loads issued ahead of the write-back's stores, slot end offsets by DPP, nontemporal window loads stopping at the chunk's last byte, nontemporal write-back; chunks by guided self-scheduling from 4M literals, fixed 96-literal chunks below; fills and long-literal phase: body steps with no fit tests while >= 31 bits are left (29 with the 12-bit table), then the wave fills' tails as four masked lookups with no fit test per code (checked steps only for a 14..30-bit code or a cut code in the tail), a lane's first literal's tail from the word saved where its body ended and its status carried from that tail, and the other kernels' checked tails (the long phase's at its refill points); long literals one lane each streaming from HBM after the fills, dense ranges listed longest-first; literals of >= 8 KiB by a whole workgroup in speculative pieces; compacted-output form: wave fills packed per workgroup from an LDS cursor into a bound layout made from the input offsets, each lane storing its two literals in unaligned 16-byte pieces; small-call mode: a persistent kernel behind a host-mapped doorbell); encode v5 (byte-balanced workgroup ranges, start map and DPP segmented scan, run accumulator, LDS image, live chunks only; packed form: length pass, length scan, the same kernel into exact positions; string literals v1: length pass + form step, length scan, a tile kernel that writes prefix, H bit and the Huffman or raw payload); string-literal decode v1 (parse kernel, Huffman payloads gathered by the ordered pack, the packed form's region decode, merge, length scan, ordered pack with a source per string); block scan v1 (count pass, length scans, emit pass: one lane per block); block apply v1 (one wave per decoder: lane-parallel look and stage, records resolved in order against a ring in LDS); frame scan v1 (count pass, length scans, emit pass: one lane per connection; fragments gathered by the ordered pack); block plan v1 (a default-and-hash pass, then one wave per encoder: headers resolved in order against a hashed ring in LDS, 64 entries a search step, matches confirmed on bytes); frame write v1 (length scan, status pass, a tile kernel that makes each 16-byte chunk of the wire: frame headers in registers, payloads by the pack's aligned loads)"

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
    hpk_h2_set_frames_device(&hpk_frames_device);  // hpk_h2_read_frames' way to the device frame scan (hpk_internal.h)
    hpk_h2_set_write_device(&hpk_write_device);    // hpk_h2_write_headers' way to the device frame write
    return c;
}

int hpk_grow(void** p, size_t* cap, size_t need) {
    if (need <= *cap) return HPK_E_OK;
    size_t n = need + need / 4 + 4096;
    (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    HIP_TRY(hipMalloc(p, n));
    *cap = n;
    return HPK_E_OK;
}

// The per-stream slots (hpk_calls.h says what the three do; hpk_slot, hpk_device.h, has the rules they keep).
int hpk_slot_acquire(hpk_ctx* c, hpk_slot** slot) {
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

int hpk_slot_reserve(hpk_ctx* c, hpk_slot* s, std::initializer_list<hpk_slot_need> needs) {
    bool small = false;
    for (const hpk_slot_need& nd : needs) small |= nd.buf->cap < nd.bytes;
    if (small) {
        if (s->ev_set)
            HIP_TRY(hipEventSynchronize(s->ev));
        else if (s->used)
            HIP_TRY(hipStreamSynchronize(c->own));
        for (const hpk_slot_need& nd : needs)
            if (int rc = hpk_grow(&nd.buf->p, &nd.buf->cap, nd.bytes)) return rc;
    }
    s->used = true;
    return HPK_E_OK;
}

int hpk_slot_commit(hpk_ctx* c, hpk_slot* s) {
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
        s.each_buf([](DevBuf& b) { (void)hipFree(b.p); });
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

int hpk_take_err(hpk_ctx* c) {
    if (!__atomic_exchange_n(c->h_err, 0u, __ATOMIC_ACQ_REL)) return HPK_E_OK;
    return hpk_set_err_msg("a batch had non-monotone offsets or offsets past a blob's capacity (HPK_BAD_OFFSETS)",
                           HPK_E_INVAL);
}

extern "C" int hpk_ctx_check(hpk_ctx* c) {
    if (!c) return HPK_E_INVAL;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return hpk_take_err(c);
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
