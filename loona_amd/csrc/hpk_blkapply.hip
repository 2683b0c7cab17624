// hpk_blkapply.hip — the header-block apply's own kernel (hpk_apply_blocks): the table-dependent half of
// Decoder::decode_with_cb (crates/loona-hpack/src/decoder.rs:368-450; the table: crates/loona-hpack/src/lib.rs:
// 43-289) for many decoders at once. A translation unit of its own. One wave per decoder, one decoder per
// workgroup; the table is the one serial dependency, everything else is lane-parallel:
//   * the look: the lanes walk the decoder's list 64 blocks at a time, each lane its block's records
//     (check_record, hpk_blkapply.h): a bad input makes the decoder void, a size update above 32 * lim sets the
//     list position from which its blocks are deferred. Both are known before anything is applied, so a void or
//     deferred block never touches the table. (One lane walks a whole block here, as in the scan: two dependent
//     loads per record of a very long block while its neighbours wait.)
//   * the apply, per block, per chunk of 64 records: stage_record per lane (one 16-byte load and the strings'
//     three arrays), then apply_record for each record in turn on words broadcast by readlane against the ring in
//     LDS, each emitted header kept by the lane of its position; then one 16-byte store per lane. The block's
//     result goes out at its end, the table once at the decoder's end.
// A chunk does not run over a block's end (the simple form: DESIGN.md §4.1h), so a block of 28 fields leaves 36
// lanes idle in the stage and the store. The ring holds kRing 16-byte records, 32 KiB: five workgroups per CU.
#include "hpk_device.h"
#include "hpk_blkapply.h"

namespace {

constexpr uint32_t kRing = 2048;  // records of a decoder's ring in LDS (hpk_test_blkapply_geometry): 32 * kRing = 64 KiB of table
constexpr uint32_t kChunk = 64;   // field records staged at a time, one per lane
constexpr uint32_t kWgDecs = 1;   // decoders per workgroup, one wave each

struct ApplyArgs {
    const uint4* fields;
    const uint32_t* field_off;
    uint32_t nblocks;
    const uint32_t* out_off;
    const uint32_t* out_len;
    const uint8_t* status;
    uint32_t nstrs;
    uint32_t str_base, static_base;
    const uint32_t* dec_blk_off;
    const uint32_t* dec_blk;
    uint32_t ndecs;
    hpk_dtab* tabs;
    uint4* tab_ent;
    uint64_t tab_ent_cap;
    uint4* headers;
    uint32_t headers_cap;
    uint32_t* results;  // four words per block
    const hpk_header* stat;
    uint32_t* err;
};

// The decoder's table as hpk_blkapply.h takes it: entry i (newest first) is ring[(head + i) mod kRing]. Every
// lane runs this with the same values; lane 0 alone stores a push (a wave's LDS operations keep their order, so
// every lane's later get sees it).
struct Ring {
    uint4* ring;
    uint32_t head, count, size, max_size, max_allowed;
    __device__ __forceinline__ hpk_header get(uint32_t i) const {
        const uint4 v = ring[(head + i) & (kRing - 1u)];
        return hpk_header{v.x, v.y, v.z, v.w};
    }
    __device__ __forceinline__ void push(const hpk_header& h) {
        head = (head - 1u) & (kRing - 1u);
        if (threadIdx.x == 0u) ring[head] = make_uint4(h.name_off, h.name_len, h.value_off, h.value_len);
        count += 1u;
    }
    __device__ __forceinline__ void pop() { count -= 1u; }
    __device__ __forceinline__ void clear() { count = 0u; }
};

__device__ __forceinline__ uint32_t bcast(uint32_t v, uint32_t lane) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}

// a block's result, lanes 0 to 3 one word each
__device__ __forceinline__ void put_result(uint32_t* results, uint32_t b, uint32_t lane, uint32_t first, uint32_t n,
                                           uint32_t error, uint32_t detail) {
    if (lane < 4u) results[4u * (size_t)b + lane] = lane == 0u ? first : lane == 1u ? n : lane == 2u ? error : detail;
}

__global__ __launch_bounds__(64) void hpk_blkapply(ApplyArgs a) {
    __shared__ uint4 ring[kRing];
    const uint32_t d = blockIdx.x, lane = threadIdx.x;
    hpk_dtab* const tab = a.tabs + d;
    const uint32_t ent = tab->ent, cap = tab->cap, count0 = tab->count, maxsz0 = tab->max_size;
    const uint32_t l0 = a.dec_blk_off[d], l1 = a.dec_blk_off[d + 1], lend = a.dec_blk_off[a.ndecs];
    const bool list_ok = l0 <= l1 && l1 <= lend;
    const uint32_t n = list_ok ? l1 - l0 : 0u;  // the listed blocks
    const uint32_t lim = cap < kRing ? cap : kRing;
    const uint32_t limit = 32u * lim;  // the largest table the ring holds

    // ---- the look: bad inputs, and the first list position with a size update the ring cannot hold
    bool bad = !list_ok || (uint64_t)ent + cap > a.tab_ent_cap || count0 > cap;
    uint32_t kdef = n;
    for (uint32_t k0 = 0; k0 < n; k0 += 64u) {  // 64 listed blocks at a time, a lane walking its block's records
        bool big = false;
        if (k0 + lane < n) {
            const uint32_t b = a.dec_blk[l0 + k0 + lane];
            uint32_t lo = 0u, hi = 0u;
            bool ok = false;
            if (b < a.nblocks) {
                lo = a.field_off[b];
                hi = a.field_off[b + 1];
                ok = lo <= hi && hi <= a.headers_cap;
            }
            bad |= !ok;
            if (ok)
                for (uint32_t i = lo; i < hi; ++i) {
                    const uint4 f = a.fields[i];
                    bool bg;
                    bad |= !hpkapp::check_record(f.x, f.y, f.z, a.out_off, a.out_len, a.nstrs, a.str_base, limit, &bg);
                    big |= bg;
                }
        }
        const unsigned long long any_big = __ballot(big);
        if (kdef == n && any_big) kdef = k0 + (uint32_t)__ffsll((long long)any_big) - 1u;
    }

    if (__any(bad)) {  // void: every listed block deferred, the table untouched
        for (uint32_t k = lane; k < n; k += 64u) {
            const uint32_t b = a.dec_blk[l0 + k];
            if (b >= a.nblocks) continue;
            uint32_t* r = a.results + 4u * (size_t)b;
            r[0] = a.field_off[b];
            r[1] = 0u;
            r[2] = HPK_BLK_DEFERRED;
            r[3] = 0u;
        }
        if (lane == 0u) {
            tab->applied = 0u;
            *a.err = 1u;
        }
        return;
    }

    // ---- the apply
    const uint32_t napply = (maxsz0 > limit || count0 > lim) ? 0u : kdef;
    if (napply) {
        for (uint32_t i = lane; i < count0; i += 64u) ring[i] = a.tab_ent[(size_t)ent + i];
        __syncthreads();
    }
    Ring t{ring, 0u, count0, tab->size, maxsz0, tab->max_allowed};
    for (uint32_t k0 = 0; k0 < napply; k0 += 64u) {
        uint32_t bl = 0u, lo = 0u, hi = 0u;
        if (k0 + lane < napply) {
            bl = a.dec_blk[l0 + k0 + lane];
            lo = a.field_off[bl];
            hi = a.field_off[bl + 1];
        }
        const uint32_t m = napply - k0 < 64u ? napply - k0 : 64u;
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t b = bcast(bl, j), lo_j = bcast(lo, j), hi_j = bcast(hi, j);
            hpkapp::Blk blk = {0u, 0, 0, 0u};
            bool stopped = false;
            for (uint32_t c = lo_j; c < hi_j && !stopped; c += kChunk) {
                const uint32_t nrec = hi_j - c < kChunk ? hi_j - c : kChunk;
                hpkapp::Rec r = {0u, 0u, 0u, 0u, 0u, 0u};
                if (lane < nrec) {
                    const uint4 f = a.fields[c + lane];
                    r = hpkapp::stage_record(f.x, f.y, f.z, a.out_off, a.out_len, a.status, a.str_base);
                }
                uint4 mine = make_uint4(0u, 0u, 0u, 0u);
                uint32_t nemit = 0u;
                for (uint32_t i = 0; i < nrec; ++i) {
                    const hpkapp::Rec u = {bcast(r.index, i),    bcast(r.ctl, i),       bcast(r.name_off, i),
                                           bcast(r.name_len, i), bcast(r.value_off, i), bcast(r.value_len, i)};
                    hpk_header h;
                    const hpkapp::Step s = hpkapp::apply_record(t, a.stat, a.static_base, u, blk, &h);
                    if (s == hpkapp::kStop) {
                        stopped = true;
                        break;
                    }
                    if (s == hpkapp::kEmit) {
                        if (lane == nemit) mine = make_uint4(h.name_off, h.name_len, h.value_off, h.value_len);
                        nemit += 1u;
                    }
                }
                // the chunk's headers: lo_j + n_headers <= hi_j <= headers_cap
                if (lane < nemit) a.headers[(size_t)lo_j + (blk.n_headers - nemit) + lane] = mine;
                if (hi_j - c <= kChunk) break;
            }
            if (!stopped) hpkapp::finish_block(blk);
            put_result(a.results, b, lane, lo_j, blk.n_headers, (uint32_t)blk.error, (uint32_t)blk.detail);
        }
    }
    // the deferred rest of the list
    for (uint32_t k = napply + lane; k < n; k += 64u) {
        const uint32_t b = a.dec_blk[l0 + k];
        uint32_t* r = a.results + 4u * (size_t)b;
        r[0] = a.field_off[b];
        r[1] = 0u;
        r[2] = HPK_BLK_DEFERRED;
        r[3] = 0u;
    }
    if (napply) {  // the table goes back in the input layout: linear, newest first (count <= lim <= cap)
        __syncthreads();
        const uint32_t cnt = t.count < cap ? t.count : cap;
        for (uint32_t i = lane; i < cnt; i += 64u) a.tab_ent[(size_t)ent + i] = ring[(t.head + i) & (kRing - 1u)];
        if (lane == 0u) {
            tab->count = cnt;
            tab->size = t.size;
            tab->max_size = t.max_size;
        }
    }
    if (lane == 0u) tab->applied = napply;
}
}  // namespace

static_assert(sizeof(hpk_header) == 16 && sizeof(hpk_block_result) == 16 && sizeof(hpk_dtab) == 32, "record sizes");

int hpk_launch_blkapply(hpk_ctx* c, const hpk_field* fields, const uint32_t* field_off, uint32_t nblocks, const uint32_t* out_off,
                        const uint32_t* out_len, const uint8_t* status, uint32_t nstrs, uint32_t str_base, uint32_t static_base,
                        const uint32_t* dec_blk_off, const uint32_t* dec_blk, uint32_t ndecs, hpk_dtab* tabs, hpk_header* tab_ent,
                        uint64_t tab_ent_cap, hpk_header* headers, uint32_t headers_cap, hpk_block_result* results,
                        const hpk_header* d_static) {
    ApplyArgs a{};
    a.fields = reinterpret_cast<const uint4*>(fields);
    a.field_off = field_off;
    a.nblocks = nblocks;
    a.out_off = out_off;
    a.out_len = out_len;
    a.status = status;
    a.nstrs = nstrs;
    a.str_base = str_base;
    a.static_base = static_base;
    a.dec_blk_off = dec_blk_off;
    a.dec_blk = dec_blk;
    a.ndecs = ndecs;
    a.tabs = tabs;
    a.tab_ent = reinterpret_cast<uint4*>(tab_ent);
    a.tab_ent_cap = tab_ent_cap;
    a.headers = reinterpret_cast<uint4*>(headers);
    a.headers_cap = headers_cap;
    a.results = reinterpret_cast<uint32_t*>(results);
    a.stat = d_static;
    a.err = c->d_err;
    hipLaunchKernelGGL(hpk_blkapply, dim3(ndecs / kWgDecs), dim3(64u * kWgDecs), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}

extern "C" int hpk_test_blkapply_geometry(uint32_t* ring_entries, uint32_t* chunk_fields, uint32_t* wg_decoders) {
    if (!ring_entries || !chunk_fields || !wg_decoders) return HPK_E_INVAL;
    *ring_entries = kRing;
    *chunk_fields = kChunk;
    *wg_decoders = kWgDecs;
    return HPK_E_OK;
}
