// hpk_calls_strings.hip — the string-literal entry points of the C ABI (include/hpk.h): lengths, encode and decode.
#include "hpk_calls.h"

// The string-literal lengths alone (include/hpk.h): the length pass and its form step, no scratch.
extern "C" int hpk_string_len_batch(hpk_ctx* c, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off, uint32_t n,
                                    const uint8_t* policy, uint32_t* out_len, int flags) {
    if (int rc = hpk_check_call(c, !in_off || (n && !out_len), flags, n, "string-length call", nullptr, nullptr)) return rc;
    if (n == 0) return HPK_E_OK;
    if (!in_blob && in_cap) return hpk_set_err_msg("null blob", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    hpk_in_or_codes(c, &in_blob, &in_cap);
    int rc;
    if ((rc = hpk_launch_enclen(c, in_blob, hpk_clamp_cap(in_cap), in_off, n, out_len, nullptr)) ||
        (rc = hpk_launch_strlen_form(c, hpk_clamp_cap(in_cap), in_off, n, policy, out_len, nullptr)))
        return rc;
    return hpk_call_end(c, flags);
}

int hpk_strings_steps(hpk_ctx* c, hpk_slot* s, size_t tmp, const uint8_t* in_blob, uint32_t in_cap, const uint32_t* in_off,
                      uint32_t n, const uint8_t* policy, uint8_t* out_blob, uint32_t out_cap, uint32_t* out_off,
                      uint32_t* out_len, uint8_t* status) {
    hpk_in_or_codes(c, &in_blob, &in_cap);
    hpk_out_or_tmp(s, tmp, &out_blob, &out_cap);
    int rc;
    if ((rc = hpk_launch_enclen(c, in_blob, in_cap, in_off, n, out_len, nullptr)) ||
        (rc = hpk_launch_strlen_form(c, in_cap, in_off, n, policy, out_len, status)) ||
        (rc = hpk_len_scan(c, out_len, n, out_off, s->pk_tmp.p)))
        return rc;
    const hpk_batch b{in_blob, in_cap, in_off, n, out_blob, out_cap, out_off, out_len, status};
    return hpk_launch_encode_strings(c, b, policy, hpk_len_scan_verdict(s->pk_tmp.p, n));
}

// The end of a packed host form, its arrays' copies back already queued: the wait, the total read from the caller's
// out_off[n], exactly the bytes written (no more than out_cap) from the staging buffer's output region, the slot
// used, then bad offsets (HPK_E_INVAL) before a result that did not fit (HPK_E_NOSPACE).
static int packed_host_end(hpk_ctx* c, hpk_slot* s, const hpk_stage& g, hpk_at<uint8_t> out, const uint32_t* out_off_n,
                           uint8_t* out_blob, size_t out_cap) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t total = *out_off_n, give = total < out_cap ? total : out_cap;
    if (give) {
        HIP_TRY(g.back(out_blob, out, give));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    int rc;
    if ((rc = hpk_slot_commit(c, s)) || (rc = hpk_take_err(c))) return rc;
    if (total > out_cap) return hpk_set_err_msg("the packed bytes pass the output capacity", HPK_E_NOSPACE);
    return HPK_E_OK;
}

// The host form: offsets and policies checked before anything is copied, the input staged into the slot's
// scratch in one piece, the steps, out_off[n] read back, then exactly the bytes written and the three arrays.
static int strings_host(hpk_ctx* c, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off, uint32_t n,
                        const uint8_t* policy, uint8_t* out_blob, size_t out_cap, uint32_t* out_off, uint32_t* out_len,
                        uint8_t* status) {
    if (hpk_check_offsets(in_off, n, in_cap)) return HPK_E_INVAL;
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
    const uint32_t dcap = hpk_clamp_cap(bound < out_cap ? (size_t)bound : out_cap);
    const hpk_lay_strings l = hpk_layout_strings(in_bytes, n, dcap);
    const size_t tmp = hpk_pack_tmp_bytes(n);
    hpk_slot* s;
    int rc;
    if ((rc = hpk_slot_acquire(c, &s)) || (rc = hpk_slot_reserve(c, s, {{&s->pk_tmp, tmp + 32}, {&s->str_stage, l.bytes}})))
        return rc;
    const hpk_stage g{c->stream, s->str_stage.as<uint8_t>()};
    HIP_TRY(g.up_range(l.in, in_blob, in_off[0], in_bytes));
    HIP_TRY(g.up(l.ioff, in_off, (size_t)n + 1));
    if (policy) HIP_TRY(g.up(l.pol, policy, n));
    if ((rc = hpk_strings_steps(c, s, tmp, g(l.in), (uint32_t)in_bytes, g(l.ioff), n, policy ? g(l.pol) : nullptr, g(l.out), dcap,
                                g(l.ooff), g(l.len), g(l.st))))
        return rc;
    HIP_TRY(g.back(out_off, l.ooff, (size_t)n + 1));
    HIP_TRY(g.back(out_len, l.len, n));
    HIP_TRY(g.back(status, l.st, n));
    return packed_host_end(c, s, g, l.out, out_off + n, out_blob, out_cap);
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
    if (n == 0) return hpk_packed_empty(c, out_off, out_cap, flags);
    const size_t tmp = hpk_pack_tmp_bytes(n);
    hpk_slot* s;
    int rc;
    if ((rc = hpk_slot_acquire(c, &s)) || (rc = hpk_slot_reserve(c, s, {{&s->pk_tmp, tmp + 32}}))) return rc;
    if ((rc = hpk_strings_steps(c, s, tmp, in_blob, hpk_clamp_cap(in_cap), in_off, n, policy, out_blob, hpk_clamp_cap(out_cap),
                            out_off, out_len, status)))
        return rc;
    if ((rc = hpk_slot_commit(c, s))) return rc;
    return hpk_packed_end(c, out_off + n, out_cap, flags);
}

int hpk_strdec_reserve(hpk_ctx* c, hpk_slot* s, uint32_t in_cap, uint32_t n, uint64_t need, size_t stage, hpk_strdec_scratch* k) {
    size_t tmp = hpk_bound_tmp_bytes(n);  // (the scans follow each other: one scratch)
    if (tmp < hpk_pack_tmp_bytes(n)) tmp = hpk_pack_tmp_bytes(n);
    const size_t words = 4 * (size_t)n + 4;
    if (int rc = hpk_slot_reserve(c, s, {{&s->long_list, 4 * (size_t)n}, {&s->pk_bound, 4 * ((size_t)n + 1)}, {&s->pk_tmp, tmp},
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

int hpk_strdec_steps(hpk_ctx* c, hpk_slot* s, const hpk_strdec_scratch& k, uint64_t need, const uint8_t* in_blob, uint32_t in_cap,
                     const uint32_t* str_off, const uint32_t* str_end, uint32_t n, uint8_t* out_blob, uint32_t out_cap,
                     uint32_t* out_off, uint32_t* out_len, uint32_t* consumed, uint8_t* status) {
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
    const uint32_t dcap = hpk_clamp_cap(bound < out_cap ? (size_t)bound : out_cap);
    const hpk_lay_strdec l = hpk_layout_strdec(dev_in, n, dcap, mirror);
    hpk_slot* s;
    hpk_strdec_scratch k;
    int rc;
    if ((rc = hpk_slot_acquire(c, &s)) || (rc = hpk_strdec_reserve(c, s, dev_in, n, need, l.bytes, &k))) return rc;
    const hpk_stage g{c->stream, s->sd_stage.as<uint8_t>()};
    HIP_TRY(g.up_range(l.in, in_blob, lo, hi));
    HIP_TRY(g.up(l.off, str_off, (size_t)n + (mirror ? 1 : 0)));
    if (!mirror) HIP_TRY(g.up(l.end, str_end, n));
    if ((rc = hpk_strdec_steps(c, s, k, need, g(l.in), dev_in, g(l.off), g(l.end), n, g(l.out), dcap, g(l.ooff), g(l.len), g(l.con),
                               g(l.st))))
        return rc;
    HIP_TRY(g.back(out_off, l.ooff, (size_t)n + 1));
    HIP_TRY(g.back(out_len, l.len, n));
    if (consumed) HIP_TRY(g.back(consumed, l.con, n));
    HIP_TRY(g.back(status, l.st, n));
    return packed_host_end(c, s, g, l.out, out_off + n, out_blob, out_cap);
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
    const uint64_t need = (uint64_t)hpk_decoded_bound(hpk_clamp_cap(in_cap)) + 4ull * n;
    if (need > HPK_MAX_OFFSET) return hpk_set_err_msg("the string-literal decode's output would pass 4 GiB", HPK_E_INVAL);
    if (n == 0) return hpk_packed_empty(c, out_off, out_cap, flags);
    hpk_slot* s;
    hpk_strdec_scratch k;
    int rc;
    if ((rc = hpk_slot_acquire(c, &s)) || (rc = hpk_strdec_reserve(c, s, hpk_clamp_cap(in_cap), n, need, 0, &k))) return rc;
    if ((rc = hpk_strdec_steps(c, s, k, need, in_blob, hpk_clamp_cap(in_cap), str_off, str_end ? str_end : str_off + 1, n, out_blob,
                           hpk_clamp_cap(out_cap), out_off, out_len, consumed, status)))
        return rc;
    if ((rc = hpk_slot_commit(c, s))) return rc;
    return hpk_packed_end(c, out_off + n, out_cap, flags);
}
