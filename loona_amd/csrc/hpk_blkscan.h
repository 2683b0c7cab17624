// hpk_blkscan.h — the per-lane code of the header-block scan (hpk_blkscan.hip, hpk_scan_blocks): the table-free
// half of Decoder::decode_with_cb (crates/loona-hpack/src/decoder.rs:368-450) on one block blob[a .. e): the
// field kind from the first octet, decode_integer (decoder.rs:67-125) with the kind's prefix, and for a literal
// (decode_literal, decoder.rs:502-527) the name string when the index is 0, then the value string, each framed
// by str_parse (hpk_strparse.h: decode_string's front half, decoder.rs:135-143) against the rest of the block.
// Where fields and strings lie never depends on table state, so a block is walked with no decoder in hand.
// The walk stops at the block's end or at the first integer or length error, which it records in the last field
// with the stage (index, name, value) at which the reference would raise it.
//
// One walk serves both passes: it counts fields and listed strings itself and hands every field record and every
// string window to a visitor. The count pass passes a visitor that does nothing, the emit pass one that stores;
// the two cannot disagree on what is where. Nothing here touches memory except through the pointer it is given,
// so tests/emu/blkscan_emu.cpp runs this code as it is on the host.
//
// Loads are byte loads, as hpk_strparse.h's and for its reasons. A string's payload is never read. An octet is
// read only after it is known to lie inside the block, and the block inside the blob (the caller's check).
#pragma once
#include <stdint.h>

#include "../../include/hpk.h"
#include "hpk_strparse.h"

namespace hpkblk {

struct IntParse {
    uint32_t err;   // HPK_BLK_OK, HPK_BLK_INT_TOO_MANY_OCTETS or HPK_BLK_INT_NOT_ENOUGH_OCTETS
    uint32_t v;     // the value (at most mask + 2^28 - 1)
    uint32_t used;  // its octets, 1 to 5
};

// decode_integer on blob[a .. e), a < e, b0 = blob[a], mask = 2^prefix - 1
template <class BP>
__device__ __forceinline__ IntParse int_parse(BP blob, uint32_t a, uint32_t e, uint32_t b0, uint32_t mask) {
    IntParse r = {HPK_BLK_OK, b0 & mask, 1u};
    if (r.v < mask) return r;
    const uint32_t w = e - a;
    bool done = false;
#pragma unroll
    for (uint32_t k = 1; k < 5u; ++k) {  // up to four more octets, 7 bits each, low bits first
        if (done) break;
        if (k >= w) {  // the block ends inside the integer
            r.err = HPK_BLK_INT_NOT_ENOUGH_OCTETS;
            return r;
        }
        const uint32_t b = blob[a + k];
        r.used = k + 1u;
        r.v += (b & 127u) << (7u * (k - 1u));
        if (!(b & 128u)) {
            done = true;
        } else if (r.used == 5u) {  // the continuation bit still set on the 5th octet
            r.err = HPK_BLK_INT_TOO_MANY_OCTETS;
            return r;
        }
    }
    return r;
}

// str_parse's status as the block decoder reports it
__device__ __forceinline__ uint32_t str_err(uint32_t status) {
    return status == HPK_OK                        ? (uint32_t)HPK_BLK_OK
           : status == HPK_PREFIX_TOO_MANY_OCTETS ? (uint32_t)HPK_BLK_INT_TOO_MANY_OCTETS
           : status == HPK_STRING_NOT_ENOUGH_OCTETS ? (uint32_t)HPK_BLK_STR_NOT_ENOUGH_OCTETS
                                                   : (uint32_t)HPK_BLK_INT_NOT_ENOUGH_OCTETS;
}

struct Counts {
    uint32_t fields, strs;
};

// the count pass's visitor
struct NoVisit {
    __device__ __forceinline__ void field(uint32_t, const hpk_field&) {}
    __device__ __forceinline__ void string(uint32_t, uint32_t, uint32_t) {}
};

// The block blob[a .. e), a <= e and e within the blob (the caller's check). vis.string(s, off, end): the
// block's s-th listed string has the exact window [off, end); vis.field(i, f): its i-th field, f.str the
// block-relative index of the field's first listed string. A field's strings are handed over before the field.
template <class BP, class V>
__device__ __forceinline__ Counts walk_block(BP blob, uint32_t a, uint32_t e, V& vis) {
    Counts n = {0u, 0u};
    uint32_t pos = a;
    while (pos < e) {
        const uint32_t b0 = blob[pos];
        hpk_field f;
        f.kind = (uint8_t)((b0 & 128u) ? HPK_FIELD_INDEXED
                           : (b0 & 64u) ? HPK_FIELD_LIT_INCR
                           : (b0 & 32u) ? HPK_FIELD_SIZE_UPDATE
                           : (b0 & 16u) ? HPK_FIELD_LIT_NEVER
                                        : HPK_FIELD_LIT_PLAIN);
        const uint32_t mask = (b0 & 128u) ? 127u : (b0 & 64u) ? 63u : (b0 & 32u) ? 31u : 15u;
        const IntParse ip = int_parse(blob, pos, e, b0, mask);
        f.index = ip.err ? 0u : ip.v;  // (no value without its last octet)
        f.str = n.strs;
        f.nstr = 0;
        f.err = (uint8_t)ip.err;
        f.err_stage = 0;
        f.at = pos;
        uint32_t at = pos + ip.used;
        if (!ip.err && f.kind != HPK_FIELD_INDEXED && f.kind != HPK_FIELD_SIZE_UPDATE) {
            // decode_literal: the name string when the index is 0, then the value string
            for (uint32_t stage = ip.v == 0u ? 1u : 2u; stage <= 2u; ++stage) {
                const hpkstr::StrParse sp = hpkstr::str_parse(blob, e, at, e);
                if (sp.status != HPK_OK) {
                    f.err = (uint8_t)str_err(sp.status);
                    f.err_stage = (uint8_t)stage;
                    break;
                }
                vis.string(n.strs, at, at + sp.consumed);
                n.strs += 1u;
                f.nstr += 1u;
                at += sp.consumed;
            }
        }
        vis.field(n.fields, f);
        n.fields += 1u;
        if (f.err) break;
        pos = at;
    }
    return n;
}

}  // namespace hpkblk
