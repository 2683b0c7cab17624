// hpk_blkplan.hip — the header-block plan's kernels (hpk_plan_blocks): the table half of Encoder::encode
// (crates/loona-hpack/src/encoder.rs:210-264; find_header crates/loona-hpack/src/lib.rs:261-288; the table
// lib.rs:43-164) for many encoders at once, the mirror of hpk_blkapply.hip. A translation unit of its own.
//   * hpk_blkplan_hash, one lane per header, 256-lane workgroups: the header's defaults (kind HPK_PLAN_NONE, three
//     empty verbatim items) and the hashes of its name and value into scratch, which takes the hashing off the
//     serial chain below. A string whose offsets are bad hashes to 0 and is not read.
//   * hpk_blkplan, one wave per encoder, one encoder per workgroup. The look: the lanes check the table record, the
//     list, the listed blocks' headers (a lane a block) and the carried-in entries (a lane an entry); a bad input
//     makes the encoder void before anything is written. Then the table goes into the ring in LDS, each carried-in
//     entry hashed by the lane that loads it, and lane l keeps static entry l with its hashes in registers. Per
//     block, per chunk of 64 headers, the lanes stage the references and hashes; the headers are resolved in turn
//     on words broadcast by readlane: the search runs over groups of 64 entries in ascending index order (the static
//     ones, then the ring newest first), each lane testing one entry (hpkplan::test_entry: lengths, hashes, then the
//     bytes), two ballots per group (hpkplan::combine); a new name is pushed by lane 0. The lane of a header's
//     position keeps its record and items and stores them once per chunk. The table goes back once.
// A chunk does not run over a block's end, as in the apply. The ring holds kRing records of 24 bytes (an hpk_header
// and the two hashes), 48 KiB: three workgroups per CU.
#include "hpk_device.h"
#include "hpk_blkplan.h"

namespace {

constexpr uint32_t kRing = 2048;  // records of an encoder's ring in LDS (hpk_test_blkplan_geometry): 32 * kRing = 64 KiB of table
constexpr uint32_t kChunk = 64;   // headers staged at a time, one per lane
constexpr uint32_t kWgEncs = 1;   // encoders per workgroup, one wave each
constexpr uint32_t kHashWg = 256;

struct PlanArgs {
    uint8_t* arena;
    uint32_t arena_cap, static_base, fields_base, prefix_base;
    const uint32_t* field_off;
    const uint32_t* hdr_off;
    uint32_t nblocks, hdrs_cap;
    const uint32_t* enc_blk_off;
    const uint32_t* enc_blk;
    const uint8_t* enc_flags;
    uint32_t nencs;
    hpk_dtab* tabs;
    uint4* tab_ent;
    uint64_t tab_ent_cap;
    uint4* reps;
    uint32_t* item_off;
    uint32_t* item_len;
    uint8_t* item_policy;
    uint2* hashes;  // per header: the name's, the value's
    const hpk_header* stat;
    uint32_t* err;
};

struct ArenaBytes {
    const uint8_t* p;
    __device__ __forceinline__ uint32_t operator()(uint32_t at) const { return p[at]; }
};

__device__ __forceinline__ void put_out(const PlanArgs& a, uint32_t j, const hpkplan::Out& o) {
    a.reps[j] = make_uint4(o.rep[0], o.rep[1], o.rep[2], o.rep[3]);
    for (uint32_t k = 0; k < 3u; ++k) {
        a.item_off[3u * (size_t)j + k] = o.off[k];
        a.item_len[3u * (size_t)j + k] = o.len[k];
        a.item_policy[3u * (size_t)j + k] = (uint8_t)o.pol[k];
    }
}

__global__ __launch_bounds__(kHashWg) void hpk_blkplan_hash(PlanArgs a) {
    const uint32_t j = blockIdx.x * kHashWg + threadIdx.x;
    if (j >= a.hdrs_cap) return;
    put_out(a, j, hpkplan::defaults());
    const uint32_t f0 = a.field_off[2u * (size_t)j], f1 = a.field_off[2u * (size_t)j + 1], f2 = a.field_off[2u * (size_t)j + 2];
    const ArenaBytes by{a.arena};
    uint2 h = make_uint2(0u, 0u);
    if (f0 <= f1 && (uint64_t)a.fields_base + f1 <= a.arena_cap) h.x = hpkplan::hash(by, a.fields_base + f0, f1 - f0);
    if (f1 <= f2 && (uint64_t)a.fields_base + f2 <= a.arena_cap) h.y = hpkplan::hash(by, a.fields_base + f1, f2 - f1);
    a.hashes[j] = h;
}

// The encoder's table as hpkapp::insert and evict take it: entry i (newest first) is record (head + i) mod kRing.
// Every lane runs this with the same values; lane 0 alone stores a push (a wave's LDS operations keep their order,
// so every lane's later read sees it). nh / vh: the hashes of the header a push is about to add.
struct Ring {
    uint4* ring;
    uint2* rh;
    uint32_t head, count, size, max_size, nh, vh;
    __device__ __forceinline__ hpk_header get(uint32_t i) const {
        const uint4 v = ring[(head + i) & (kRing - 1u)];
        return hpk_header{v.x, v.y, v.z, v.w};
    }
    __device__ __forceinline__ hpkplan::Ent ent(uint32_t i) const {
        const uint32_t at = (head + i) & (kRing - 1u);
        const uint4 v = ring[at];
        const uint2 h = rh[at];
        return hpkplan::Ent{hpk_header{v.x, v.y, v.z, v.w}, h.x, h.y};
    }
    __device__ __forceinline__ void push(const hpk_header& h) {
        head = (head - 1u) & (kRing - 1u);
        if (threadIdx.x == 0u) {
            ring[head] = make_uint4(h.name_off, h.name_len, h.value_off, h.value_len);
            rh[head] = make_uint2(nh, vh);
        }
        count += 1u;
    }
    __device__ __forceinline__ void pop() { count -= 1u; }
    __device__ __forceinline__ void clear() { count = 0u; }
};

__device__ __forceinline__ uint32_t bcast(uint32_t v, uint32_t lane) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}

__global__ __launch_bounds__(64) void hpk_blkplan(PlanArgs a) {
    __shared__ uint4 ring[kRing];
    __shared__ uint2 rh[kRing];
    const uint32_t e = blockIdx.x, lane = threadIdx.x;
    hpk_dtab* const tab = a.tabs + e;
    const uint32_t ent = tab->ent, cap = tab->cap, count0 = tab->count, maxsz0 = tab->max_size;
    const uint32_t l0 = a.enc_blk_off[e], l1 = a.enc_blk_off[e + 1], lend = a.enc_blk_off[a.nencs];
    const bool list_ok = l0 <= l1 && l1 <= lend;
    const uint32_t n = list_ok ? l1 - l0 : 0u;  // the listed blocks
    const uint32_t lim = cap < kRing ? cap : kRing;
    const uint32_t limit = 32u * lim;  // the largest table the ring holds
    const ArenaBytes by{a.arena};

    // ---- the look: bad inputs
    const bool tab_ok = (uint64_t)ent + cap <= a.tab_ent_cap && count0 <= cap;
    bool bad = !list_ok || !tab_ok;
    for (uint32_t k = lane; k < n; k += 64u) {  // a lane walking its block's headers
        const uint32_t b = a.enc_blk[l0 + k];
        uint32_t lo = 0u, hi = 0u;
        bool ok = false;
        if (b < a.nblocks) {
            lo = a.hdr_off[b];
            hi = a.hdr_off[b + 1];
            ok = lo <= hi && hi <= a.hdrs_cap;
        }
        bad |= !ok;
        if (ok)
            for (uint32_t j = lo; j < hi; ++j)
                bad |= !hpkplan::check_header(a.field_off[2u * (size_t)j], a.field_off[2u * (size_t)j + 1],
                                              a.field_off[2u * (size_t)j + 2], a.fields_base, a.arena_cap);
    }
    if (tab_ok)
        for (uint32_t i = lane; i < count0; i += 64u) {
            const uint4 v = a.tab_ent[(size_t)ent + i];
            bad |= !hpkplan::check_entry(hpk_header{v.x, v.y, v.z, v.w}, a.arena_cap);
        }
    if (__any(bad)) {  // void: the table untouched, its blocks' headers keep their defaults
        if (lane == 0u) {
            tab->applied = 0u;
            *a.err = 1u;
        }
        return;
    }
    if (maxsz0 > limit || count0 > lim) {  // deferred: the ring cannot hold the table
        if (lane == 0u) tab->applied = 0u;
        return;
    }

    // ---- the table into the ring, the static entries into registers
    for (uint32_t i = lane; i < count0; i += 64u) {
        const uint4 v = a.tab_ent[(size_t)ent + i];
        ring[i] = v;
        rh[i] = make_uint2(hpkplan::hash(by, v.x, v.y), hpkplan::hash(by, v.z, v.w));
    }
    __syncthreads();
    hpkplan::Ent se = {hpk_header{0u, 0u, 0u, 0u}, 0u, 0u};
    const bool has_static = lane < hpkplan::kStaticEntries;
    if (has_static) {
        se.h = a.stat[lane];
        se.h.name_off += a.static_base;
        se.h.value_off += a.static_base;
        se.nh = hpkplan::hash(by, se.h.name_off, se.h.name_len);
        se.vh = hpkplan::hash(by, se.h.value_off, se.h.value_len);
    }
    const uint32_t policy = (a.enc_flags[e] & 1u) ? HPK_STR_AUTO : HPK_STR_RAW;

    // ---- the plan
    Ring t{ring, rh, 0u, count0, tab->size, maxsz0, 0u, 0u};
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t b = a.enc_blk[l0 + k];
        const uint32_t lo = a.hdr_off[b], hi = a.hdr_off[b + 1];
        for (uint32_t c = lo; c < hi; c += kChunk) {
            const uint32_t nrec = hi - c < kChunk ? hi - c : kChunk;
            hpkplan::Ent q = {hpk_header{0u, 0u, 0u, 0u}, 0u, 0u};
            if (lane < nrec) {
                const size_t j = (size_t)c + lane;
                const uint32_t f0 = a.field_off[2u * j], f1 = a.field_off[2u * j + 1], f2 = a.field_off[2u * j + 2];
                const uint2 h = a.hashes[j];
                q = hpkplan::Ent{hpk_header{a.fields_base + f0, f1 - f0, a.fields_base + f1, f2 - f1}, h.x, h.y};
            }
            hpkplan::Out mine = hpkplan::defaults();
            for (uint32_t i = 0; i < nrec; ++i) {
                const hpkplan::Ent u = {hpk_header{bcast(q.h.name_off, i), bcast(q.h.name_len, i), bcast(q.h.value_off, i),
                                                   bcast(q.h.value_len, i)},
                                        bcast(q.nh, i), bcast(q.vh, i)};
                hpkplan::Found f = {0u, 0u};
                uint32_t m = has_static ? (uint32_t)hpkplan::test_entry(by, se, u) : 0u;
                bool done = hpkplan::combine(__ballot(m == hpkplan::kFull), __ballot(m != hpkplan::kNone), 1u, f);
                for (uint32_t g = 0; !done && g < t.count; g += hpkplan::kGroup) {
                    m = g + lane < t.count ? (uint32_t)hpkplan::test_entry(by, t.ent(g + lane), u) : 0u;
                    done = hpkplan::combine(__ballot(m == hpkplan::kFull), __ballot(m != hpkplan::kNone),
                                            hpkplan::kStaticEntries + 1u + g, f);
                }
                if (lane == i) mine = hpkplan::build(f, u.h, policy, a.prefix_base + 4u * (c + i));
                if (hpkplan::kind_of(f) == HPK_PLAN_NEW_NAME) {
                    t.nh = u.nh;
                    t.vh = u.vh;
                    hpkapp::insert(t, u.h);
                }
            }
            if (lane < nrec) {  // c + lane < hi <= hdrs_cap; the prefix area holds 4 * hdrs_cap bytes, 4-byte aligned
                put_out(a, c + lane, mine);
                *reinterpret_cast<uint32_t*>(a.arena + a.prefix_base + 4u * (size_t)(c + lane)) = mine.prefix;
            }
        }
    }
    // the table goes back in the input layout: linear, newest first (count <= lim <= cap)
    __syncthreads();
    const uint32_t cnt = t.count < cap ? t.count : cap;
    for (uint32_t i = lane; i < cnt; i += 64u) a.tab_ent[(size_t)ent + i] = ring[(t.head + i) & (kRing - 1u)];
    if (lane == 0u) {
        tab->count = cnt;
        tab->size = t.size;
        tab->max_size = t.max_size;
        tab->applied = n;
    }
}
}  // namespace

static_assert(sizeof(hpk_hrep) == 16 && sizeof(hpk_header) == 16 && sizeof(hpk_dtab) == 32, "record sizes");

int hpk_launch_blkplan(hpk_ctx* c, uint8_t* arena, uint32_t arena_cap, uint32_t static_base, uint32_t fields_base,
                       uint32_t prefix_base, const uint32_t* field_off, const uint32_t* hdr_off, uint32_t nblocks, uint32_t hdrs_cap,
                       const uint32_t* enc_blk_off, const uint32_t* enc_blk, const uint8_t* enc_flags, uint32_t nencs, hpk_dtab* tabs,
                       hpk_header* tab_ent, uint64_t tab_ent_cap, hpk_hrep* reps, uint32_t* item_off, uint32_t* item_len,
                       uint8_t* item_policy, void* hashes, const hpk_header* d_static) {
    PlanArgs a{};
    a.arena = arena;
    a.arena_cap = arena_cap;
    a.static_base = static_base;
    a.fields_base = fields_base;
    a.prefix_base = prefix_base;
    a.field_off = field_off;
    a.hdr_off = hdr_off;
    a.nblocks = nblocks;
    a.hdrs_cap = hdrs_cap;
    a.enc_blk_off = enc_blk_off;
    a.enc_blk = enc_blk;
    a.enc_flags = enc_flags;
    a.nencs = nencs;
    a.tabs = tabs;
    a.tab_ent = reinterpret_cast<uint4*>(tab_ent);
    a.tab_ent_cap = tab_ent_cap;
    a.reps = reinterpret_cast<uint4*>(reps);
    a.item_off = item_off;
    a.item_len = item_len;
    a.item_policy = item_policy;
    a.hashes = static_cast<uint2*>(hashes);
    a.stat = d_static;
    a.err = c->d_err;
    if (hdrs_cap) {
        hipLaunchKernelGGL(hpk_blkplan_hash, dim3((hdrs_cap + kHashWg - 1u) / kHashWg), dim3(kHashWg), 0, c->stream, a);
        HIP_TRY(hipGetLastError());
    }
    if (nencs && nblocks) {
        hipLaunchKernelGGL(hpk_blkplan, dim3(nencs / kWgEncs), dim3(64u * kWgEncs), 0, c->stream, a);
        HIP_TRY(hipGetLastError());
    }
    return HPK_E_OK;
}

namespace {
__global__ __launch_bounds__(kHashWg) void hpk_blkplan_boff(const uint32_t* out_off, const uint32_t* hdr_off, uint32_t nblocks,
                                                            uint32_t* boff) {
    const uint32_t b = blockIdx.x * kHashWg + threadIdx.x;
    if (b <= nblocks) boff[b] = out_off[3u * (size_t)hdr_off[b]];
}
}  // namespace

int hpk_launch_blkplan_boff(hpk_ctx* c, const uint32_t* out_off, const uint32_t* hdr_off, uint32_t nblocks, uint32_t* boff) {
    hipLaunchKernelGGL(hpk_blkplan_boff, dim3(nblocks / kHashWg + 1u), dim3(kHashWg), 0, c->stream, out_off, hdr_off, nblocks, boff);
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}

extern "C" int hpk_test_blkplan_geometry(uint32_t* ring_entries, uint32_t* chunk_headers, uint32_t* wg_encoders,
                                         uint32_t* search_group) {
    if (!ring_entries || !chunk_headers || !wg_encoders || !search_group) return HPK_E_INVAL;
    *ring_entries = kRing;
    *chunk_headers = kChunk;
    *wg_encoders = kWgEncs;
    *search_group = hpkplan::kGroup;
    return HPK_E_OK;
}

extern "C" int hpk_test_blkplan_hash(const uint8_t* blob, const uint32_t* off, uint32_t n, uint32_t* out) {
    if (n && (!blob || !off || !out)) return HPK_E_INVAL;
    struct HostBytes {
        const uint8_t* p;
        uint32_t operator()(uint32_t at) const { return p[at]; }
    };
    for (uint32_t i = 0; i < n; ++i) {
        if (off[i + 1] < off[i]) return HPK_E_INVAL;
        out[i] = hpkplan::hash(HostBytes{blob}, off[i], off[i + 1] - off[i]);
    }
    return HPK_E_OK;
}
