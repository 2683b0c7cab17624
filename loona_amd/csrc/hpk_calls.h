// hpk_calls.h — what the host call layer's units share: hpk_ctx.hip (the context and the slots), hpk_calls_batch.hip,
// hpk_calls_strings.hip and hpk_calls_blocks.hip (the entry points of the C ABI, include/hpk.h). None of them has a
// kernel or launches one; the kernel units include hpk_device.h only.
#pragma once
#include <initializer_list>

#include "hpk_device.h"
#include "hpk_layout.h"

// hpk_ctx.hip. The per-stream slots: hpk_slot (hpk_device.h) has the rules these three keep. acquire: the slot of the
// context's current stream, claimed or taken over if it has none. reserve: the buffers a call is about to use, each of
// at least its bytes; if any must grow, the slot's last launch is waited for first (once), through its event or else the
// own stream. commit: after the call's last operation on the stream, the slot's event recorded there.
struct hpk_slot_need {
    DevBuf* buf;
    size_t bytes;
};
int hpk_slot_acquire(hpk_ctx* c, hpk_slot** slot);
int hpk_slot_reserve(hpk_ctx* c, hpk_slot* s, std::initializer_list<hpk_slot_need> needs);
int hpk_slot_commit(hpk_ctx* c, hpk_slot* s);
int hpk_grow(void** p, size_t* cap, size_t need);  // a grow-only device allocation (nothing of it may be in flight)
int hpk_take_err(hpk_ctx* c);  // read and clear the sticky device error flag (the ctx stream must be synchronised)

// hpk_calls_batch.hip.
int hpk_check_offsets(const uint32_t* off, uint32_t n, size_t cap);
uint32_t hpk_clamp_cap(size_t cap);  // to HPK_MAX_OFFSET
uint32_t hpk_clamp_u32(size_t x);
// The argument checks that the compacted form, the packed forms and the pack share; `what` names the caller in
// the messages. in_cap (the two decodes): *need = the bytes that hold every literal's 4-rounded decoded bound.
int hpk_check_call(const hpk_ctx* c, bool null_arg, int flags, uint32_t n, const char* what, const size_t* in_cap, uint64_t* need);
// the end of a device-pointer call: an asynchronous one returns, a synchronous one waits and reports bad offsets
int hpk_call_end(hpk_ctx* c, int flags);
// The end of a packed call: a synchronous one waits, then reports bad offsets (HPK_E_INVAL) before a result that
// did not fit (HPK_E_NOSPACE: dst_off[n] read back with the wait).
int hpk_packed_end(hpk_ctx* c, const uint32_t* dst_off_n, size_t dst_cap, int flags);

// A packed call of no literals: out_off[0] = 0 on the device, then the call's end.
static inline int hpk_packed_empty(hpk_ctx* c, uint32_t* out_off, size_t out_cap, int flags) {
    HIP_TRY(hipMemsetAsync(out_off, 0, 4, c->stream));
    return hpk_packed_end(c, out_off, out_cap, flags);
}

// Blobs of no bytes: addresses that exist for the kernels' base pointers. The input's clamped loads still read one
// chunk, so they get the code table; with a capacity of 0 no byte of the output is written: the 16-byte boundary
// behind the scan's `tmp` bytes of pk_tmp (reserved with tmp + 32).
template <class Cap>
static inline void hpk_in_or_codes(const hpk_ctx* c, const uint8_t** in_blob, Cap* in_cap) {
    if (!*in_blob || !*in_cap) *in_blob = reinterpret_cast<const uint8_t*>(c->d_codes), *in_cap = 0;
}
template <class Cap>
static inline void hpk_out_or_tmp(const hpk_slot* s, size_t tmp, uint8_t** out_blob, Cap* out_cap) {
    if (!*out_blob || !*out_cap) *out_blob = s->pk_tmp.as<uint8_t>() + ((tmp + 15) & ~(size_t)15), *out_cap = 0;
}

// hpk_calls_strings.hip, for the block paths. The string-literal encode's steps on device arrays (s: the stream's
// slot, pk_tmp reserved with tmp + 32 bytes): the length pass and its form step write out_len and status, the length
// scan out_off, and the emit kernel every representation at its final place, clipped at out_cap.
int hpk_strings_steps(hpk_ctx* c, hpk_slot* s, size_t tmp, const uint8_t* in_blob, uint32_t in_cap, const uint32_t* in_off,
                      uint32_t n, const uint8_t* policy, uint8_t* out_blob, uint32_t out_cap, uint32_t* out_off,
                      uint32_t* out_len, uint8_t* status);
// The string-literal decode's scratch on one stream's slot: the parse step's arrays and the gather's offsets in
// sd_meta, the gathered Huffman blob, and what the packed decode uses (region scratch, bound layout, scans, list).
struct hpk_strdec_scratch {
    uint32_t *start, *hlen, *rlen, *hoff;
    uint8_t *pst, *sel, *hblob;
};
// (stage: the bytes of the host form's staging buffer, 0 for device pointers)
int hpk_strdec_reserve(hpk_ctx* c, hpk_slot* s, uint32_t in_cap, uint32_t n, uint64_t need, size_t stage, hpk_strdec_scratch* k);
// The string-literal decode's steps on device arrays (hpk_decode_strings.hip has the list), s the stream's slot,
// reserved by hpk_strdec_reserve. need: hpk_decoded_bound(in_cap) + 4 n, the region scratch's bytes.
int hpk_strdec_steps(hpk_ctx* c, hpk_slot* s, const hpk_strdec_scratch& k, uint64_t need, const uint8_t* in_blob, uint32_t in_cap,
                     const uint32_t* str_off, const uint32_t* str_end, uint32_t n, uint8_t* out_blob, uint32_t out_cap,
                     uint32_t* out_off, uint32_t* out_len, uint32_t* consumed, uint8_t* status);

// A staging buffer on the context's stream, its regions named by a layout (hpk_layout.h): copies of `count` elements
// up into a region and back from one, none issued for a count of 0. The region states the element width.
struct hpk_stage {
    hipStream_t stream;
    uint8_t* d;
    template <class T>
    T* operator()(hpk_at<T> r) const { return r.in(d); }
    template <class T>
    hipError_t up(hpk_at<T> r, const T* src, size_t count) const {
        return count ? hipMemcpyAsync(r.in(d), src, count * sizeof(T), hipMemcpyHostToDevice, stream) : hipSuccess;
    }
    template <class T>
    hipError_t back(T* dst, hpk_at<T> r, size_t count) const {
        return count ? hipMemcpyAsync(dst, r.in(d), count * sizeof(T), hipMemcpyDeviceToHost, stream) : hipSuccess;
    }
    // the bytes [lo, hi) of a blob whose offsets stay absolute
    hipError_t up_range(hpk_at<uint8_t> r, const uint8_t* src, size_t lo, size_t hi) const {
        return hi > lo ? hipMemcpyAsync(r.in(d) + lo, src + lo, hi - lo, hipMemcpyHostToDevice, stream) : hipSuccess;
    }
};
