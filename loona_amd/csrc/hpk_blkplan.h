// hpk_blkplan.h — the per-header code of the header-block plan (hpk_blkplan.hip, hpk_plan_blocks): the table half
// of Encoder::encode (crates/loona-hpack/src/encoder.rs:210-264) with HeaderTable::find_header (crates/loona-hpack/
// src/lib.rs:261-288) and add_header / consolidate_table (lib.rs:108-142; hpkapp::insert and evict, hpk_blkapply.h),
// without the string coding. A name or a value is a reference (offset, length) into the call's one arena; unlike the
// apply, the plan reads the bytes behind a reference, through a byte accessor the caller supplies (by(at) is the
// arena's octet at `at`): the arena in device memory in the kernel, a vector in tests/emu/blkplan_emu.cpp, which
// compiles this file as it is. Nothing here uses a builtin or touches memory except through what it is given.
//
// The steps, per lane and wave-uniform apart so that an emulation can run the 64 lanes in a loop:
//   * hash, per lane: the 32-bit filter of a string. It only filters: test_entry confirms every match on bytes;
//   * test_entry, per lane: one table entry against the header in hand: no match, the name, or name and value;
//   * combine, wave-uniform: the two ballots of a group of 64 consecutive entries (ascending indices) into the
//     search's running answer: the lowest index that matches whole, which ends the search, else the highest index
//     whose name matches (find_header's "last name match");
//   * kind_of, prefix_octets, build, per lane: the representation, its first octets, the record and three items.
#pragma once
#include <stdint.h>

#include "../../include/hpk.h"
#include "hpk_blkapply.h"

// (hpk_test_blkplan_hash runs the hash on the host, so under the HIP compiler everything here is host and device code)
#ifdef __HIP__
#define HPKPLAN_FN __host__ __device__ __forceinline__
#else
#define HPKPLAN_FN __device__ __forceinline__
#endif

namespace hpkplan {

constexpr uint32_t kStaticEntries = hpkapp::kStaticEntries;
constexpr uint32_t kGroup = 64;  // the entries a search step tests, one per lane

// FNV-1a over the octets, then a finishing mix so that short strings spread over all 32 bits.
template <class Bytes>
HPKPLAN_FN uint32_t hash(Bytes by, uint32_t off, uint32_t n) {
    uint32_t h = 0x811C9DC5u;
    for (uint32_t i = 0; i < n; ++i) h = (h ^ by(off + i)) * 0x01000193u;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    h *= 0x297A2D39u;
    h ^= h >> 15;
    return h;
}

// A table entry as the search sees it, and the header in hand: the references and the two hashes.
struct Ent {
    hpk_header h;
    uint32_t nh, vh;
};

enum Match : uint32_t { kNone = 0, kName = 1, kFull = 2 };

template <class Bytes>
HPKPLAN_FN bool same(Bytes by, uint32_t a, uint32_t b, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i)
        if (by(a + i) != by(b + i)) return false;
    return true;
}

// One entry against the header q. Lengths and hashes first; what they let through is compared byte by byte, so the
// answer never depends on the hash.
template <class Bytes>
HPKPLAN_FN Match test_entry(Bytes by, const Ent& e, const Ent& q) {
    if (e.h.name_len != q.h.name_len || e.nh != q.nh) return kNone;
    if (!same(by, e.h.name_off, q.h.name_off, q.h.name_len)) return kNone;
    if (e.h.value_len != q.h.value_len || e.vh != q.vh) return kName;
    return same(by, e.h.value_off, q.h.value_off, q.h.value_len) ? kFull : kName;
}

HPKPLAN_FN uint32_t lowest_bit(uint64_t m) {  // m != 0
    uint32_t k = 0;
    for (uint32_t s = 32; s; s >>= 1)
        if (!(m & ((1ull << s) - 1ull))) {
            m >>= s;
            k += s;
        }
    return k;
}
HPKPLAN_FN uint32_t highest_bit(uint64_t m) {  // m != 0
    uint32_t k = 0;
    for (uint32_t s = 32; s; s >>= 1)
        if (m >> s) {
            m >>= s;
            k += s;
        }
    return k;
}

// find_header's answer, 1-based indices, 0 = none.
struct Found {
    uint32_t full, name;
};

// One group's ballots (bit l: lane l's entry, whose 1-based index is base + l; name_mask holds the whole matches
// too). Groups come in ascending order. True: a whole match, the search ends.
HPKPLAN_FN bool combine(uint64_t full_mask, uint64_t name_mask, uint32_t base, Found& f) {
    if (name_mask) f.name = base + highest_bit(name_mask);
    if (!full_mask) return false;
    f.full = base + lowest_bit(full_mask);
    return true;
}

HPKPLAN_FN uint32_t kind_of(const Found& f) {  // encoder.rs:246-264
    return f.full ? HPK_PLAN_INDEXED : f.name ? HPK_PLAN_NAME_INDEXED : HPK_PLAN_NEW_NAME;
}

// encode_integer_into (encoder.rs:93-122) for a value below 2^21 + the prefix's mask: the octets, first octet in the
// low byte, and their count (1 to 4). An index of a ring of 2^14 records or fewer takes at most 3.
HPKPLAN_FN uint32_t prefix_octets(uint32_t value, uint32_t prefix_bits, uint32_t lead, uint32_t* len) {
    const uint32_t mask = (1u << prefix_bits) - 1u;
    if (value < mask) {
        *len = 1u;
        return lead | value;
    }
    const uint32_t v = value - mask;
    uint32_t w = lead | mask;
    if (v < 128u) {
        *len = 2u;
        return w | v << 8;
    }
    w |= ((v & 127u) | 128u) << 8;
    if (v < 16384u) {
        *len = 3u;
        return w | (v >> 7) << 16;
    }
    *len = 4u;
    return w | (((v >> 7) & 127u) | 128u) << 16 | ((v >> 14) & 127u) << 24;
}

// What a header leaves: the hpk_hrep record as four words, the prefix octets as the dword that goes to the prefix
// area, and the three items (offset, length, policy).
struct Out {
    uint32_t rep[4];
    uint32_t prefix;
    uint32_t off[3], len[3], pol[3];
};

HPKPLAN_FN Out defaults() {
    Out o = {{0u, 0u, 0u, 0u}, 0u, {0u, 0u, 0u}, {0u, 0u, 0u}, {HPK_STR_VERBATIM, HPK_STR_VERBATIM, HPK_STR_VERBATIM}};
    return o;
}

// q: the header's own references; policy: the encoder's (HPK_STR_AUTO or HPK_STR_RAW); prefix_at: where this
// header's prefix dword lies in the arena.
HPKPLAN_FN Out build(const Found& f, const hpk_header& q, uint32_t policy, uint32_t prefix_at) {
    Out o = defaults();
    const uint32_t kind = kind_of(f);
    uint32_t index = 0u, plen = 1u;
    if (kind == HPK_PLAN_INDEXED) {
        index = f.full;
        o.prefix = prefix_octets(index, 7u, 0x80u, &plen);
    } else if (kind == HPK_PLAN_NAME_INDEXED) {
        index = f.name;
        o.prefix = prefix_octets(index, 4u, 0x00u, &plen);
        o.off[1] = q.value_off, o.len[1] = q.value_len, o.pol[1] = policy;
    } else {
        o.prefix = 0x40u;
        o.off[1] = q.name_off, o.len[1] = q.name_len, o.pol[1] = policy;
        o.off[2] = q.value_off, o.len[2] = q.value_len, o.pol[2] = policy;
    }
    o.off[0] = prefix_at, o.len[0] = plen;
    o.rep[0] = index;
    o.rep[1] = kind | plen << 8;
    o.rep[2] = o.prefix;
    return o;
}

// Whether header j's two strings lie in the arena: field_off[2j] <= [2j+1] <= [2j+2] and fields_base + the last
// within arena_cap.
HPKPLAN_FN bool check_header(uint32_t f0, uint32_t f1, uint32_t f2, uint32_t fields_base, uint64_t arena_cap) {
    return f0 <= f1 && f1 <= f2 && (uint64_t)fields_base + f2 <= arena_cap;
}
HPKPLAN_FN bool check_entry(const hpk_header& h, uint64_t arena_cap) {
    return (uint64_t)h.name_off + h.name_len <= arena_cap && (uint64_t)h.value_off + h.value_len <= arena_cap;
}

}  // namespace hpkplan
