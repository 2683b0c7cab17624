// hpk_blkapply.h — the per-record code of the header-block apply (hpk_blkapply.hip, hpk_apply_blocks): the
// table-dependent half of Decoder::decode_with_cb (crates/loona-hpack/src/decoder.rs:368-450; the table:
// crates/loona-hpack/src/lib.rs:43-289) over the records hpk_scan_blocks left and the results
// hpk_decode_strings_packed left for its string list. No byte of any string is touched: a name or a value is a
// reference (offset, length) into one arena the caller defines, a table entry is an hpk_header of such references,
// and so is an emitted header. The order of the checks is apply_block's (hpk_hdec.cpp, the host's one apply pass), which states the
// reference's precedence.
//
// Two steps:
//   * stage_record, per lane, table-free: one hpk_field and the out_off / out_len / status of its one or two
//     strings become a Rec: the value's reference, the name's reference when the index is 0, the error the scan
//     recorded at the index stage, and the first error of the literal's strings (the scan's framing errors and the
//     Huffman statuses, name before value);
//   * apply_record, wave-uniform, in field order: the lookup (static records for 1 to 61, the table above), the
//     checks, the insertion with its evictions, the size update.
// The table is a type the caller supplies (count, size, max_size, max_allowed; get(i) the i-th newest entry,
// push(h) a new newest one, pop() drops the oldest, clear()): an LDS ring in the kernel, a plain array in
// tests/emu/blkapply_emu.cpp, which compiles this file as it is. Nothing here uses a builtin or touches memory
// except through what it is given.
#pragma once
#include <stdint.h>

#include "../../include/hpk.h"

namespace hpkapp {

constexpr uint32_t kStaticEntries = 61;  // RFC 7541 App. A

// One staged record: what apply_record needs of a field, every word of it known without the table.
struct Rec {
    uint32_t index;  // hpk_field.index
    uint32_t ctl;    // kind | e0 << 8 | el << 16 | dl << 24: the error recorded at the index stage; the literal's
                     // first string error (hpk_block_error) and its detail (hpk_status for HPK_BLK_STR_HUFFMAN)
    uint32_t name_off, name_len;    // the name string's reference (index 0 only)
    uint32_t value_off, value_len;  // the value string's reference
};

__device__ __forceinline__ bool is_literal(uint32_t kind) {
    return kind != HPK_FIELD_INDEXED && kind != HPK_FIELD_SIZE_UPDATE;
}

// The field record as four words (x index, y str, z kind | nstr << 8 | err << 16 | err_stage << 24, w at), the
// strings' arrays, and where the packed strings lie in the arena. A string is read only if the field lists it
// (str + nstr is inside the arrays: the caller's check); a literal whose record lists fewer strings than it needs
// (no scan writes one) fails as a Huffman error with HPK_BAD_OFFSETS.
template <class U32P, class U8P>
__device__ __forceinline__ Rec stage_record(uint32_t fx, uint32_t fy, uint32_t fz, U32P out_off, U32P out_len, U8P status,
                                            uint32_t str_base) {
    const uint32_t kind = fz & 255u, nstr = (fz >> 8) & 255u, err = (fz >> 16) & 255u, stage = fz >> 24;
    Rec r = {fx, kind, 0u, 0u, 0u, 0u};
    if (err && stage == 0u) {
        r.ctl |= err << 8;
        return r;
    }
    if (!is_literal(kind)) return r;
    uint32_t s = fy, left = nstr, el = 0u, dl = 0u;
    if (fx == 0u) {  // the name string
        if (err && stage == 1u) {
            el = err;
        } else if (!left) {
            el = HPK_BLK_STR_HUFFMAN, dl = HPK_BAD_OFFSETS;
        } else {
            const uint32_t st = status[s];
            if (st) el = HPK_BLK_STR_HUFFMAN, dl = st;
            r.name_off = str_base + out_off[s];
            r.name_len = out_len[s];
            s += 1u;
            left -= 1u;
        }
    }
    if (!el) {  // the value string
        if (err && stage == 2u) {
            el = err;
        } else if (!left) {
            el = HPK_BLK_STR_HUFFMAN, dl = HPK_BAD_OFFSETS;
        } else {
            const uint32_t st = status[s];
            if (st) el = HPK_BLK_STR_HUFFMAN, dl = st;
            r.value_off = str_base + out_off[s];
            r.value_len = out_len[s];
        }
    }
    r.ctl |= el << 16 | dl << 24;
    return r;
}

// A block's running result.
struct Blk {
    uint32_t n_headers;
    int32_t error, detail;
    uint32_t last_size_update;  // the last record applied was a size update (SizeUpdateAtEnd, decoder.rs:445-447)
};

enum Step : uint32_t { kNext = 0, kEmit = 1, kStop = 2 };

__device__ __forceinline__ uint64_t entry_size(const hpk_header& h) {  // RFC 7541 §4.1, in 64 bits
    return (uint64_t)h.name_len + h.value_len + 32u;
}

// DynamicTable::consolidate_table (lib.rs:124-142): the oldest entries go while the size passes the limit
template <class Tab>
__device__ __forceinline__ void evict(Tab& t, uint64_t incoming) {
    while ((uint64_t)t.size + incoming > t.max_size) {
        if (!t.count) {  // (a size the caller handed in without its entries)
            t.size = 0u;
            break;
        }
        t.size -= (uint32_t)entry_size(t.get(t.count - 1u));
        t.pop();
    }
}

// add_header (lib.rs:108-122): an entry larger than the limit empties the table and adds nothing
template <class Tab>
__device__ __forceinline__ void insert(Tab& t, const hpk_header& h) {
    const uint64_t sz = entry_size(h);
    if (sz > t.max_size) {
        t.clear();
        t.size = 0u;
        return;
    }
    evict(t, sz);
    t.push(h);
    t.size += (uint32_t)sz;
}

// HeaderTable::get_from_table (lib.rs:228-255): 1-based, the static entries, then the table, newest first. stat:
// the 61 static records with offsets relative to the static text, which lies at static_base of the arena.
template <class Tab, class SP>
__device__ __forceinline__ bool lookup(const Tab& t, SP stat, uint32_t static_base, uint32_t index, hpk_header* h) {
    if (index == 0u) return false;
    const uint32_t ri = index - 1u;
    if (ri < kStaticEntries) {
        *h = stat[ri];
        h->name_off += static_base;
        h->value_off += static_base;
        return true;
    }
    const uint32_t di = ri - kStaticEntries;
    if (di >= t.count) return false;
    *h = t.get(di);
    return true;
}

__device__ __forceinline__ Step fail(Blk& b, uint32_t error, uint32_t detail) {
    b.error = (int32_t)error;
    b.detail = (int32_t)detail;
    return kStop;
}

// One record against the table, apply_block's order. kEmit: *out is the block's next header (b.n_headers counts
// it); kStop: b holds the block's error and nothing after this record is applied.
template <class Tab, class SP>
__device__ __forceinline__ Step apply_record(Tab& t, SP stat, uint32_t static_base, const Rec& r, Blk& b, hpk_header* out) {
    const uint32_t kind = r.ctl & 255u, e0 = (r.ctl >> 8) & 255u, el = (r.ctl >> 16) & 255u, dl = r.ctl >> 24;
    b.last_size_update = kind == HPK_FIELD_SIZE_UPDATE;
    if (e0) return fail(b, e0, 0u);
    if (kind == HPK_FIELD_INDEXED) {
        if (!lookup(t, stat, static_base, r.index, out)) return fail(b, HPK_BLK_HEADER_INDEX_OUT_OF_BOUNDS, 0u);
        b.n_headers += 1u;
        return kEmit;
    }
    if (kind == HPK_FIELD_SIZE_UPDATE) {  // update_max_dynamic_size (decoder.rs:537-554)
        if (t.max_allowed != HPK_DTAB_NO_LIMIT && r.index > t.max_allowed) return fail(b, HPK_BLK_INVALID_MAX_DYNAMIC_SIZE, 0u);
        t.max_size = r.index;
        evict(t, 0u);
        return kNext;
    }
    // a literal: the name (its own string, or the table's: read before the insertion evicts anything, RFC 7541
    // §4.4), then the value
    hpk_header h;
    if (r.index == 0u) {
        h.name_off = r.name_off;
        h.name_len = r.name_len;
    } else if (!lookup(t, stat, static_base, r.index, &h)) {
        return fail(b, HPK_BLK_HEADER_INDEX_OUT_OF_BOUNDS, 0u);
    }
    if (el) return fail(b, el, dl);
    h.value_off = r.value_off;
    h.value_len = r.value_len;
    *out = h;
    b.n_headers += 1u;
    if (kind == HPK_FIELD_LIT_INCR) insert(t, h);
    return kEmit;
}

// The end of a block that no record stopped.
__device__ __forceinline__ void finish_block(Blk& b) {
    if (b.last_size_update) (void)fail(b, HPK_BLK_SIZE_UPDATE_AT_END, 0u);
}

// The table-free look at one record for the caller's two early decisions: *big, a size update above `limit` (the
// block is deferred); the return value, whether the record's strings lie inside the arrays of nstrs entries and
// their places in the arena below 2^32 (else the decoder is void).
template <class U32P>
__device__ __forceinline__ bool check_record(uint32_t fx, uint32_t fy, uint32_t fz, U32P out_off, U32P out_len, uint32_t nstrs,
                                             uint32_t str_base, uint32_t limit, bool* big) {
    const uint32_t kind = fz & 255u, nstr = (fz >> 8) & 255u;
    *big = kind == HPK_FIELD_SIZE_UPDATE && fx > limit;
    if ((uint64_t)fy + nstr > nstrs) return false;
    if (!is_literal(kind)) return true;
    bool ok = true;
    for (uint32_t k = 0; k < nstr && k < 2u; ++k)
        ok = ok && (uint64_t)str_base + out_off[fy + k] + out_len[fy + k] <= 0xFFFFFFFFull;
    return ok;
}

}  // namespace hpkapp
