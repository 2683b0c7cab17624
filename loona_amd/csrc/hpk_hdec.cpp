// hpk_hdec.cpp — two-pass HPACK header-block decoding around the batched Huffman kernel
// (SURVEY §8f-1). Host code: the C ABI's hpk_hdec_* entry points (include/hpk.h).
//
// Reference: hpack::Decoder, crates/loona-hpack/src/decoder.rs:257-555, with its header table
// (crates/loona-hpack/src/lib.rs:43-289). Huffman results never depend on dynamic-table state,
// so the work splits in three:
//   1. scan (per block): walk the field representations (decoder.rs:368-450) with decode_integer
//      (decoder.rs:67-125) and the string framing of decode_string (decoder.rs:135-163): record
//      every field and the byte span of every string; stop at the first integer / length error;
//   2. one Huffman batch for the H-bit strings of ALL blocks (device: hpk_decode_batch through a
//      context; or the library's CPU batch path when the caller passes no context);
//   3. apply (per block, in order per decoder): table lookups, insertions, size updates and the
//      emitted header list, reporting the FIRST error in field order exactly as the reference's
//      single pass would (index integer, then name string or name index, then value string;
//      Huffman status of a string where the reference would have decoded it).
// The opt-in device paths replace pass 1 (HPK_BLOCK_SCAN_DEVICE) or all three (HPK_BLOCK_APPLY_DEVICE); pass 3 is
// written once, apply_block, over a view of whichever scan's records.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <pthread.h>
#include <thread>
#include <vector>

#include "../../include/hpk.h"
#include "hpk_hpack.h"
#include "hpk_internal.h"  // the context's calls that are not in the C ABI: the chunked host batch, the device paths
#include "hpk_layout.h"

namespace {

// A fixed set of worker threads for the block calls' parallel passes (spawning 15 threads per
// pass cost more than a small pass). One call at a time uses it; a concurrent caller (loona's
// runtime threads each decode their own connections) spawns its own threads instead.
class Pool {
  public:
    static constexpr int kMax = 16;
    // fn(t) for t in [0, n): t = 0 on the calling thread
    void run(int n, const std::function<void(int)>& fn) {
        if (n <= 1) {
            fn(0);
            return;
        }
        std::unique_lock<std::mutex> busy(use_, std::try_to_lock);
        if (!busy.owns_lock()) {  // in use by another caller
            std::vector<std::thread> th;
            for (int t = 1; t < n; ++t) th.emplace_back(fn, t);
            fn(0);
            for (auto& x : th) x.join();
            return;
        }
        {
            std::lock_guard<std::mutex> g(m_);
            while ((int)th_.size() < kMax - 1) {
                const int id = (int)th_.size() + 1;
                th_.emplace_back([this, id] { work(id); });
            }
            job_ = &fn;
            n_ = n;
            pending_ = n - 1;
            ++gen_;
        }
        cv_.notify_all();
        fn(0);
        std::unique_lock<std::mutex> g(m_);
        done_.wait(g, [this] { return pending_ == 0; });
        job_ = nullptr;
    }
    ~Pool() {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& x : th_) x.join();
    }

  private:
    void work(int id) {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(int)>* job;
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                if (id >= n_) continue;
                job = job_;
            }
            (*job)(id);
            std::lock_guard<std::mutex> g(m_);
            if (--pending_ == 0) done_.notify_one();
        }
    }
    std::mutex use_, m_;
    std::condition_variable cv_, done_;
    std::vector<std::thread> th_;
    const std::function<void(int)>* job_ = nullptr;
    int n_ = 0, pending_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
};

// One pool per process. After a fork the child inherits the parent's Pool object but none of its
// threads (run() would wait forever for them), and maybe a mutex some parent thread held: the
// pthread_atfork child handler forgets it (leaked, never destroyed: its std::thread handles are
// meaningless in the child) and the child's first call makes a fresh one.
static Pool* g_pool = nullptr;

Pool& pool() {
    static const bool registered = [] {
        pthread_atfork(nullptr, nullptr, [] { __atomic_store_n(&g_pool, (Pool*)nullptr, __ATOMIC_RELEASE); });
        return true;
    }();
    (void)registered;
    Pool* p = __atomic_load_n(&g_pool, __ATOMIC_ACQUIRE);
    if (p) return *p;
    Pool* fresh = new Pool();  // no threads until its first run()
    Pool* expect = nullptr;
    if (__atomic_compare_exchange_n(&g_pool, &expect, fresh, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) return *fresh;
    delete fresh;  // another thread installed one first
    return *expect;
}

typedef std::function<void(const std::function<void(int)>&)> Parallel;

struct Timer {  // wall time since it was made, for the per-pass figures under HPK_HDEC_TIMING
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    long us() const {
        return (long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    }
};

// decode_integer (decoder.rs:67-125): prefix 1..8, at most 5 octets.
int decode_integer(const uint8_t* p, size_t n, int prefix, uint64_t* value, size_t* consumed) {
    if (prefix < 1 || prefix > 8) return HPK_BLK_INT_INVALID_PREFIX;
    if (n == 0) return HPK_BLK_INT_NOT_ENOUGH_OCTETS;
    const uint32_t mask = prefix == 8 ? 0xFFu : ((1u << prefix) - 1u);
    uint64_t v = p[0] & mask;
    if (v < mask) {
        *value = v;
        *consumed = 1;
        return HPK_BLK_OK;
    }
    size_t total = 1;
    unsigned m = 0;
    for (size_t i = 1; i < n; ++i) {
        const uint8_t b = p[i];
        total += 1;
        v += (uint64_t)(b & 127u) << m;
        m += 7;
        if (!(b & 128u)) {
            *value = v;
            *consumed = total;
            return HPK_BLK_OK;
        }
        if (total == 5) return HPK_BLK_INT_TOO_MANY_OCTETS;
    }
    return HPK_BLK_INT_NOT_ENOUGH_OCTETS;
}

struct Str {
    uint32_t off;       // absolute offset of the string bytes in the blocks buffer
    uint32_t len;
    uint32_t lit : 31;  // index among its scan thread's Huffman strings (huff only; + that thread's base)
    uint32_t huff : 1;
    Str() : off(0), len(0), lit(0), huff(0) {}
};

// Stages of one field in the reference's order; a scan error is recorded with the stage at which
// the reference would have raised it (hpk_field.err_stage holds the same values).
enum Stage : uint8_t { kStIndex = 0, kStName = 1, kStValue = 2 };

struct Field {  // 32 bytes (40 until round 3): a batch's fields are written once by the scan and read once by
                // the apply
    uint32_t index = 0;  // header index / name index / new table size (decode_integer's <= 5 octets: < 2^29)
    Str name, value;
    int8_t err = HPK_BLK_OK;  // scan error in this field (the last field scanned)
    uint8_t kind = HPK_FIELD_INDEXED;  // hpk_field_kind
    Stage err_stage = kStIndex;
};
static_assert(sizeof(Field) <= 32, "Field packing");

struct Scan {  // a block's fields: pools[pool][first .. first + n) (one field pool per host thread)
    uint32_t pool = 0, first = 0, n = 0;
    uint32_t lit_end = 0;  // its scan thread's Huffman strings so far, this block's included
};

// decode_string's framing (decoder.rs:135-163) without the Huffman step; a Huffman string joins its scan thread's
// list (hoff, hlen).
int scan_string(const uint8_t* base, size_t pos, size_t end, Str* s, size_t* consumed, std::vector<uint32_t>* hoff,
                std::vector<uint32_t>* hlen) {
    uint64_t len;
    size_t c;
    int e = decode_integer(base + pos, end - pos, 7, &len, &c);
    if (e) return e;
    if (c + len > end - pos) return HPK_BLK_STR_NOT_ENOUGH_OCTETS;
    s->off = (uint32_t)(pos + c);
    s->len = (uint32_t)len;
    s->huff = (base[pos] & 128u) ? 1u : 0u;
    if (s->huff) {
        s->lit = (uint32_t)hoff->size();
        hoff->push_back(s->off);
        hlen->push_back(s->len);
    }
    *consumed = c + (size_t)len;
    return HPK_BLK_OK;
}

// One block's fields appended to its scan thread's pool; the block's last field carries its scan error, if any.
void scan_block(const uint8_t* base, size_t pos, size_t end, uint32_t pool_id, std::vector<Field>* pool, Scan* out,
                std::vector<uint32_t>* hoff, std::vector<uint32_t>* hlen) {
    out->pool = pool_id;
    out->first = (uint32_t)pool->size();
    while (pos < end) {
        Field f;
        const uint8_t b = base[pos];
        f.kind = (b & 128u)  ? HPK_FIELD_INDEXED
                 : (b & 64u) ? HPK_FIELD_LIT_INCR
                 : (b & 32u) ? HPK_FIELD_SIZE_UPDATE
                 : (b & 16u) ? HPK_FIELD_LIT_NEVER
                             : HPK_FIELD_LIT_PLAIN;
        size_t c = 0;
        uint64_t v = 0;
        if (f.kind == HPK_FIELD_INDEXED || f.kind == HPK_FIELD_SIZE_UPDATE) {
            f.err = (int8_t)decode_integer(base + pos, end - pos, f.kind == HPK_FIELD_INDEXED ? 7 : 5, &v, &c);
            f.index = (uint32_t)v;
            pool->push_back(f);
            if (f.err) break;
            pos += c;
            continue;
        }
        // decode_literal (decoder.rs:502-527)
        f.err = (int8_t)decode_integer(base + pos, end - pos, f.kind == HPK_FIELD_LIT_INCR ? 6 : 4, &v, &c);
        f.index = (uint32_t)v;
        size_t at = pos + c;
        if (!f.err && f.index == 0) {
            f.err = (int8_t)scan_string(base, at, end, &f.name, &c, hoff, hlen);
            if (f.err) f.err_stage = kStName;
            at += c;
        }
        if (!f.err) {
            f.err = (int8_t)scan_string(base, at, end, &f.value, &c, hoff, hlen);
            if (f.err) f.err_stage = kStValue;
            at += c;
        }
        pool->push_back(f);
        if (f.err) break;
        pos = at;
    }
    out->n = (uint32_t)pool->size() - out->first;
    out->lit_end = (uint32_t)hoff->size();
}

}  // namespace

// RFC 7541 App. A as hpk_apply_blocks' kernel sees it (include/hpk.h): the names and values end to end, and the
// entries as references into that text.
extern "C" int hpk_static_table(const uint8_t** text, size_t* text_len, const hpk_header** entries) {
    struct Image {
        std::vector<uint8_t> text;
        hpk_header ent[61];
    };
    static const Image img = [] {
        Image m;
        for (int k = 0; k < 61; ++k) {
            const std::string_view n = hpk_static[k][0], v = hpk_static[k][1];
            const uint32_t at = (uint32_t)m.text.size(), nl = (uint32_t)n.size();
            m.ent[k] = hpk_header{at, nl, at + nl, (uint32_t)v.size()};
            m.text.insert(m.text.end(), n.begin(), n.end());
            m.text.insert(m.text.end(), v.begin(), v.end());
        }
        return m;
    }();
    if (text) *text = img.text.data();
    if (text_len) *text_len = img.text.size();
    if (entries) *entries = img.ent;
    return HPK_E_OK;
}

// Decoder state: the dynamic table (lib.rs:43-164) and the SizeUpdate limit (decoder.rs:316-318).
// The table holds its entries' bytes in one buffer, appended at the end, and the entries (offset,
// name length, value length) in a ring, newest first: an insertion or eviction allocates nothing
// (the reference's VecDeque of owned strings allocates per entry). Evicted bytes are reclaimed by
// moving the live ones (at most max_size bytes) to the buffer's start when the end is reached.
struct hpk_hdec {
    struct Ent {
        uint32_t at, nl, vl;
    };
    std::vector<Ent> ring{std::vector<Ent>(64)};  // capacity a power of two
    uint32_t first = 0, count = 0;                // newest entry at ring[first]
    std::vector<uint8_t> bytes;
    size_t end = 0;                               // bytes[0, end): entries' names and values
    size_t size = 0;
    size_t max_size = 4096;
    bool has_max_allowed = false;
    size_t max_allowed = 0;

    const Ent& at(size_t di) const { return ring[(first + di) & (ring.size() - 1)]; }
    void pop_oldest() {
        const Ent& e = at(count - 1);
        size -= (size_t)e.nl + e.vl + 32;
        count -= 1;
        if (count == 0) end = 0;
    }
    void consolidate() {
        while (size > max_size) pop_oldest();
    }
    void clear() {
        count = 0;
        size = 0;
        end = 0;
    }
    // add_header then consolidate (lib.rs:97-117): an entry larger than the limit empties the
    // table. n and v must not point into the table.
    void add(const uint8_t* n, size_t nl, const uint8_t* v, size_t vl) {
        const size_t sz = nl + vl + 32;
        if (sz > max_size) return clear();
        while (size + sz > max_size) pop_oldest();
        if (end + nl + vl > bytes.size()) {
            const size_t lo = count ? at(count - 1).at : end;  // the oldest live byte
            if (lo) {
                memmove(bytes.data(), bytes.data() + lo, end - lo);
                for (uint32_t k = 0; k < count; ++k) ring[(first + k) & (ring.size() - 1)].at -= (uint32_t)lo;
                end -= lo;
            }
            if (end + nl + vl > bytes.size()) bytes.resize(std::max<size_t>(2 * (end + nl + vl), 8192));
        }
        if (count == ring.size()) {  // grow the ring, newest first at 0
            std::vector<Ent> r(2 * ring.size());
            for (uint32_t k = 0; k < count; ++k) r[k] = at(k);
            ring.swap(r);
            first = 0;
        }
        if (nl) memcpy(bytes.data() + end, n, nl);
        if (vl) memcpy(bytes.data() + end + nl, v, vl);
        first = (first - 1) & (uint32_t)(ring.size() - 1);
        ring[first] = Ent{(uint32_t)end, (uint32_t)nl, (uint32_t)vl};
        count += 1;
        end += nl + vl;
        size += sz;
    }
    // HeaderTable::get_from_table (lib.rs:228-255): 1-based, static then dynamic
    bool get(uint64_t index, const uint8_t** n, size_t* nl, const uint8_t** v, size_t* vl) const {
        if (index == 0) return false;
        const uint64_t ri = index - 1;
        if (ri < 61) {
            *n = (const uint8_t*)hpk_static[ri][0].data();
            *nl = hpk_static[ri][0].size();
            *v = (const uint8_t*)hpk_static[ri][1].data();
            *vl = hpk_static[ri][1].size();
            return true;
        }
        const uint64_t di = ri - 61;
        if (di >= count) return false;
        const Ent& e = at((size_t)di);
        *n = bytes.data() + e.at;
        *nl = e.nl;
        *v = bytes.data() + e.at + e.nl;
        *vl = e.vl;
        return true;
    }
};

extern "C" hpk_hdec* hpk_hdec_create(void) { return new (std::nothrow) hpk_hdec(); }

extern "C" void hpk_hdec_destroy(hpk_hdec* d) { delete d; }

extern "C" int hpk_hdec_set_max_table_size(hpk_hdec* d, size_t n) {
    if (!d) return HPK_E_INVAL;
    if (d->has_max_allowed && n > d->max_allowed) return HPK_E_INVAL;  // the reference asserts
    d->max_size = n;
    d->consolidate();
    return HPK_E_OK;
}

extern "C" int hpk_hdec_set_max_allowed_table_size(hpk_hdec* d, size_t n) {
    if (!d) return HPK_E_INVAL;
    d->has_max_allowed = true;
    d->max_allowed = n;
    return HPK_E_OK;
}

extern "C" int hpk_hdec_table_size(const hpk_hdec* d, size_t* size, size_t* entries, size_t* max_size) {
    if (!d) return HPK_E_INVAL;
    if (size) *size = d->size;
    if (entries) *entries = d->count;
    if (max_size) *max_size = d->max_size;
    return HPK_E_OK;
}

namespace {

// A thread's output: header bytes and header records appended with plain copies (the vectors' sizes
// are capacities; vector::insert per string cost a fifth of the apply pass).
struct Out {
    std::vector<uint8_t> arena;
    std::vector<hpk_header> headers;
    size_t an = 0, hn = 0;  // bytes / records in use
    void reset(size_t abytes, size_t nhdr) {
        an = hn = 0;
        if (arena.size() < abytes) arena.resize(abytes);
        if (headers.size() < nhdr) headers.resize(nhdr);
    }
};

inline uint32_t put(Out& o, const void* p, size_t n) {
    const uint32_t at = (uint32_t)o.an;
    if (o.an + n > o.arena.size()) o.arena.resize(std::max(2 * o.arena.size(), o.an + n + 4096));
    if (n) memcpy(o.arena.data() + o.an, p, n);
    o.an += n;
    return at;
}

inline void put_header(Out& o, const hpk_header& h) {
    if (o.hn == o.headers.size()) o.headers.resize(2 * o.headers.size() + 1024);
    o.headers[o.hn++] = h;
}

struct Bytes {
    const uint8_t* p;
    size_t n;
};

// The default path's Huffman batch (host memory: pageable vectors or the ctx's page-locked area): string j of scan
// thread t is string lbase[t] + j of the batch.
struct Batch {
    uint32_t n = 0;                      // strings
    size_t tot = 0, otot = 0;            // their bytes, their decoded bounds (each rounded up to 4)
    std::vector<uint64_t> ibase, obase;  // each scan thread's first byte in the two blobs
    hpk_lay_hdecbatch lay;
    uint8_t *in = nullptr, *dec = nullptr, *st = nullptr;
    uint32_t *in_off = nullptr, *out_off = nullptr, *len = nullptr;
    int chunks = 0;             // device chunks under way (hpk_decode_host_begin)
    std::vector<uint32_t> cut;  // chunk j's results hold the strings below cut[j]
};

// A view of one block's scanned fields, as apply_block reads them. Both record types name a field's kind
// (hpk_field_kind), index, err and err_stage alike; a view adds, for a literal field's name (which = 0, asked for
// only when the field carries one: index == 0) and value (which = 1), the string's Huffman status and, once that is
// HPK_OK, its bytes.
//
// The host scan's: a raw string lies in the block, a Huffman string in the batch's results.
struct HostView {
    const Field* fields;
    uint32_t n;
    const uint8_t* base;  // the call's blocks
    const Batch& q;
    uint32_t lb;  // batch index of the first string of the block's scan thread
    static const Str& str(const Field& f, int which) { return which ? f.value : f.name; }
    int status(const Field& f, int which) const { return str(f, which).huff ? q.st[lb + str(f, which).lit] : 0; }
    Bytes bytes(const Field& f, int which) const {
        const Str& s = str(f, which);
        if (s.huff) return {q.dec + q.out_off[lb + s.lit], q.len[lb + s.lit]};
        return {base + s.off, s.len};
    }
};
// The device scan's (hpk_scan_blocks' records): every string, raw ones too, lies in the packed string decode's
// results (a raw string's status is HPK_OK); a field's strings are listed from f.str on, the name first.
struct DevView {
    const hpk_field* fields;
    uint32_t n;
    const hpk_blkdev& h;
    static uint32_t str(const hpk_field& f, int which) { return f.str + (which && f.index == 0 ? 1u : 0u); }
    int status(const hpk_field& f, int which) const { return h.status[str(f, which)]; }
    Bytes bytes(const hpk_field& f, int which) const { return {h.arena + h.out_off[str(f, which)], h.out_len[str(f, which)]}; }
};

// Pass 3 for one block: the reference's single pass (decoder.rs:368-450, 502-554) over the scanned fields, whichever
// scan made them. The device kernel's per-record code (hpk_blkapply.h) follows this order of checks.
template <class View>
void apply_block(hpk_hdec* d, const View& w, Out& o, hpk_block_result* r) {
    r->first_header = (uint32_t)o.hn;
    r->n_headers = 0;
    r->error = HPK_BLK_OK;
    r->detail = 0;
    auto fail = [&](int e, int detail) {
        r->error = e;
        r->detail = detail;
    };
    auto emit = [&](const uint8_t* n, size_t nl, const uint8_t* v, size_t vl) {
        hpk_header hd;
        hd.name_len = (uint32_t)nl;
        hd.name_off = put(o, n, nl);
        hd.value_len = (uint32_t)vl;
        hd.value_off = put(o, v, vl);
        put_header(o, hd);
        r->n_headers += 1;
        return hd;
    };
    bool last_was_size_update = false;
    for (uint32_t fi = 0; fi < w.n; ++fi) {
        const auto& f = w.fields[fi];
        last_was_size_update = f.kind == HPK_FIELD_SIZE_UPDATE;
        if (f.err && f.err_stage == kStIndex) return fail(f.err, 0);
        if (f.kind == HPK_FIELD_INDEXED) {
            const uint8_t *n, *v;
            size_t nl, vl;
            if (!d->get(f.index, &n, &nl, &v, &vl)) return fail(HPK_BLK_HEADER_INDEX_OUT_OF_BOUNDS, 0);
            emit(n, nl, v, vl);
            continue;
        }
        if (f.kind == HPK_FIELD_SIZE_UPDATE) {  // update_max_dynamic_size (decoder.rs:538-554)
            if (d->has_max_allowed && f.index > d->max_allowed) return fail(HPK_BLK_INVALID_MAX_DYNAMIC_SIZE, 0);
            d->max_size = (size_t)f.index;
            d->consolidate();
            continue;
        }
        // literal: name (literal string or table name), then value
        Bytes name;
        if (f.index == 0) {
            if (f.err && f.err_stage == kStName) return fail(f.err, 0);
            if (int hs = w.status(f, 0)) return fail(HPK_BLK_STR_HUFFMAN, hs);
            name = w.bytes(f, 0);
        } else {
            const uint8_t* v;
            size_t vl;
            if (!d->get(f.index, &name.p, &name.n, &v, &vl)) return fail(HPK_BLK_HEADER_INDEX_OUT_OF_BOUNDS, 0);
        }
        if (f.err && f.err_stage == kStValue) return fail(f.err, 0);
        if (int hs = w.status(f, 1)) return fail(HPK_BLK_STR_HUFFMAN, hs);
        const Bytes value = w.bytes(f, 1);
        const hpk_header hd = emit(name.p, name.n, value.p, value.n);
        // the insertion reads the header's copies in the output (the table name it came from may be
        // evicted by the insertion itself)
        if (f.kind == HPK_FIELD_LIT_INCR)
            d->add(o.arena.data() + hd.name_off, name.n, o.arena.data() + hd.value_off, value.n);
    }
    if (last_was_size_update) fail(HPK_BLK_SIZE_UPDATE_AT_END, 0);
}

// The output buffers of the last freed hpk_blocks_out (hpk_blocks_out_free), handed to the next
// call that fits in them: the caller-owned results are large (tens of MB for a big batch), and a
// fresh malloc of that size is a fresh mapping whose every page faults on first write.
struct OutCache {
    std::mutex m;
    void* p[3] = {};
    size_t cap[3] = {};  // bytes
    void* take(int k, size_t bytes) {
        {
            std::lock_guard<std::mutex> g(m);
            if (p[k] && cap[k] >= bytes) {
                void* r = p[k];
                p[k] = nullptr;
                cap[k] = 0;
                return r;
            }
        }
        return malloc(bytes ? bytes : 1);
    }
    void give(int k, void* q, size_t bytes) {
        if (!q) return;
        std::lock_guard<std::mutex> g(m);
        if (!p[k] || bytes > cap[k]) {
            free(p[k]);
            p[k] = q;
            cap[k] = bytes;
        } else {
            free(q);
        }
    }
};
OutCache g_out_cache;  // [0] arena, [1] headers, [2] block results

// Scratch of hpk_hdec_decode_blocks, kept per calling thread (loona calls from its runtime
// threads; each keeps its own): steady-state calls reuse capacity instead of page-faulting
// fresh allocations in every pass.
struct BlockScratch {
    std::vector<Scan> scans;
    std::vector<std::vector<Field>> pools;
    std::vector<std::vector<uint32_t>> thoff, thlen;
    std::vector<uint32_t> lbase, in_off, out_off, len;
    std::vector<uint8_t> st, in, dec, owner;
    std::vector<Out> outs;
    std::vector<uint64_t> bwork;  // [thread][bucket] apply work (fields + 1 per block)
    std::vector<uint8_t> bthread;  // bucket -> apply thread
    std::vector<uint16_t> bkt;     // block -> its decoder's bucket
};

// Decoders go to apply threads through kBuckets hash buckets of their addresses; the buckets are
// placed on threads longest-first by the work counted in them. (A plain hash of the
// address per thread left the busiest of 16 threads with 1.37-1.56x the mean on config 4, whose
// connections differ in size by two orders of magnitude.)
constexpr int kBucketBits = 9, kBuckets = 1 << kBucketBits;
inline uint32_t dec_bucket(const hpk_hdec* d) {
    return (uint32_t)((((uintptr_t)d >> 4) * 0x9E3779B97F4A7C15ull) >> (64 - kBucketBits));
}
thread_local BlockScratch t_scratch;

// buckets to threads, heaviest first onto the least loaded thread (W.bwork: [thread][bucket] -> W.bthread)
void place_buckets(BlockScratch& W, int nth) {
    uint64_t bsum[kBuckets];
    uint16_t order[kBuckets];
    for (int k = 0; k < kBuckets; ++k) {
        uint64_t x = 0;
        for (int t = 0; t < nth; ++t) x += W.bwork[(size_t)t * kBuckets + k];
        bsum[k] = x;
        order[k] = (uint16_t)k;
    }
    std::sort(order, order + kBuckets, [&](uint16_t x, uint16_t y) { return bsum[x] > bsum[y]; });
    uint64_t load[Pool::kMax] = {};
    W.bthread.resize(kBuckets);
    for (int i = 0; i < kBuckets; ++i) {
        int m = 0;
        for (int t = 1; t < nth; ++t)
            if (load[t] < load[m]) m = t;
        load[m] += bsum[order[i]];
        W.bthread[order[i]] = (uint8_t)m;
    }
}

// What every pass of a call shares: the call's arguments and its host threads. Thread t of a pass over the blocks
// takes [blk0(t), blk0(t + 1)) (ranges of equal block counts: ranges of equal bytes scanned slower on config 4).
struct Call {
    hpk_ctx* ctx;
    hpk_hdec* const* decs;
    const uint8_t* blocks;
    const uint32_t* block_off;
    uint32_t nblocks;
    hpk_blocks_out* out;
    int nth;
    Parallel parallel;
    bool timing;  // HPK_HDEC_TIMING: per-pass wall times to stderr
    uint32_t blk0(int t) const { return (uint32_t)((uint64_t)nblocks * t / nth); }
};

// join the per-thread outputs (W.outs, W.owner) into the caller's buffers
int join_outputs(BlockScratch& W, const Call& c) {
    const std::vector<Out>& outs = W.outs;
    hpk_blocks_out* out = c.out;
    uint32_t abase[Pool::kMax], hbase[Pool::kMax];  // each thread's first byte and first record in the joined arrays
    size_t at = 0, ht = 0;
    for (int t = 0; t < c.nth; ++t) {
        abase[t] = (uint32_t)at;
        hbase[t] = (uint32_t)ht;
        at += outs[t].an;
        ht += outs[t].hn;
    }
    out->arena_len = at;
    out->n_headers = ht;
    out->arena = (uint8_t*)g_out_cache.take(0, at);
    out->headers = (hpk_header*)g_out_cache.take(1, ht * sizeof(hpk_header));
    if (at >= (1ull << 32) || !out->arena || !out->headers) {
        hpk_blocks_out_free(out);
        return HPK_E_INVAL;
    }
    c.parallel([&](int t) {
        if (outs[t].an) memcpy(out->arena + abase[t], outs[t].arena.data(), outs[t].an);
        for (size_t j = 0; j < outs[t].hn; ++j) {
            hpk_header hd = outs[t].headers[j];
            hd.name_off += abase[t];
            hd.value_off += abase[t];
            out->headers[hbase[t] + j] = hd;
        }
        for (uint32_t b = c.blk0(t); b < c.blk0(t + 1); ++b) out->blocks[b].first_header += hbase[W.owner[b]];
    });
    return HPK_E_OK;
}

// Pass 3 of a call, for either scan. A decoder's blocks stay on one thread, in call order (decoders are independent
// of each other): the buckets are placed by the work p.work(b) states per block (fields + 1), every thread applies
// its blocks with p.apply, and the per-thread outputs are joined (a block's headers stay contiguous; blocks need not
// be in order in the arrays). A path P gives:
//   work(b)                          the block's work figure
//   headers(t)                       header records to reserve for thread t
//   apply(t, my, left, out, res)     applies block my[0] into *out and res[my[0]]; my[1 .. left) are the thread's
//                                    next blocks; nonzero (a device failure) ends the thread's pass
//   end()                            once every thread is through: the call's device work closed, the first failure
// A failure leaves the decoders as far as the pass got, and `out` empty.
template <class P>
int apply_threaded(P& p, const Call& c, long* us_apply, long* us_join) {
    const Timer t_apply;
    BlockScratch& W = t_scratch;
    const uint32_t nblocks = c.nblocks;
    const int nth = c.nth;
    if ((int)W.outs.size() < nth) W.outs.resize(nth);
    W.bwork.assign((size_t)nth * kBuckets, 0);
    W.bkt.resize(nblocks);
    c.parallel([&](int t) {
        uint64_t* const bw = W.bwork.data() + (size_t)t * kBuckets;
        for (uint32_t b = c.blk0(t); b < c.blk0(t + 1); ++b) {
            const uint32_t k = dec_bucket(c.decs[b]);
            W.bkt[b] = (uint16_t)k;
            bw[k] += p.work(b);
        }
    });
    place_buckets(W, nth);
    std::vector<Out>& outs = W.outs;
    for (int t = 0; t < nth; ++t)  // decoded headers take a few times the block bytes
        outs[t].reset(4 * (size_t)c.block_off[nblocks] / (size_t)nth + 4096, p.headers(t));
    // results go straight into the caller's malloc'd buffers (hpk_blocks_out_free)
    hpk_blocks_out* out = c.out;
    out->n_blocks = nblocks;
    out->blocks = (hpk_block_result*)g_out_cache.take(2, (size_t)nblocks * sizeof(hpk_block_result));
    int rc = out->blocks ? HPK_E_OK : HPK_E_INVAL;
    if (!rc) {
        W.owner.resize(nblocks);
        c.parallel([&](int t) {
            Out mine = std::move(outs[t]);  // (a local: no false sharing with the neighbours' headers)
            std::vector<uint32_t> my;       // this thread's blocks, in order
            my.reserve(nblocks / nth + 64);
            const uint16_t* const bk = W.bkt.data();
            const uint8_t* const bt = W.bthread.data();
            for (uint32_t b = 0; b < nblocks; ++b)
                if (bt[bk[b]] == t) {
                    my.push_back(b);
                    W.owner[b] = (uint8_t)t;
                }
            for (size_t i = 0; i < my.size(); ++i)
                if (p.apply(t, my.data() + i, my.size() - i, mine, out->blocks)) break;
            outs[t] = std::move(mine);
        });
    }
    const int end_rc = p.end();
    if (!rc) rc = end_rc;
    if (rc) {
        g_out_cache.give(2, out->blocks, (size_t)nblocks * sizeof(hpk_block_result));
        memset(out, 0, sizeof *out);
        return rc;
    }
    *us_apply = t_apply.us();
    const Timer t_join;
    rc = join_outputs(W, c);
    *us_join = t_join.us();
    return rc;
}

// The device-scan path's pass 3 (HPK_BLOCK_SCAN_DEVICE) over what hpk_blocks_device brought back (also the
// device-apply path's, for a call in which a block was deferred). Everything is back before it starts, so a device
// failure leaves every decoder as it was.
struct DevScanPath {
    const Call& c;
    const hpk_blkdev& h;
    uint32_t fields(uint32_t b) const { return h.field_off[b + 1] - h.field_off[b]; }
    uint64_t work(uint32_t b) const { return fields(b) + 1u; }
    size_t headers(int) const { return h.nfields / (size_t)c.nth + 16; }
    int apply(int, const uint32_t* my, size_t, Out& o, hpk_block_result* res) const {
        const uint32_t b = my[0];
        apply_block(c.decs[b], DevView{h.fields + h.field_off[b], fields(b), h}, o, &res[b]);
        return 0;
    }
    int end() const { return HPK_E_OK; }
};

int apply_blkdev_host(const Call& c, const hpk_blkdev& h) {
    DevScanPath p{c, h};
    long us_apply = 0, us_join = 0;
    if (int rc = apply_threaded(p, c, &us_apply, &us_join)) return rc;
    if (c.timing)
        fprintf(stderr,
                "hpk_hdec_decode_blocks: %d threads, device scan %ld us, strings %ld us, bytes back %ld us, apply %ld us, join %ld us\n",
                c.nth, h.us_scan, h.us_strings, h.us_back, us_apply, us_join);
    return HPK_E_OK;
}

// hpk_hdec_decode_blocks with HPK_BLOCK_SCAN_DEVICE (include/hpk.h has the steps): the device does the scan and
// every string; the host threads apply once everything is back.
int decode_blocks_device(const Call& c) {
    hpk_blkdev h;
    if (int rc = hpk_blocks_device(c.ctx, c.blocks, c.block_off, c.nblocks, &h)) return rc;
    return apply_blkdev_host(c, h);
}

// The device-apply path's tables as hpk_apply_blocks takes them: hpk_dtab / hpk_header records over an arena that
// is the static text, then the tables' bytes (`prior`), then the packed strings.
struct TablesOut {
    std::vector<hpk_dtab> tabs;
    std::vector<hpk_header> ent;
    std::vector<uint8_t> prior;
};
// -> false: a table does not fit the device ring
bool export_tables(const std::vector<hpk_hdec*>& decs, uint32_t ring, size_t stext_len, TablesOut* x) {
    x->tabs.resize(decs.size());
    for (size_t k = 0; k < decs.size(); ++k) {
        const hpk_hdec* d = decs[k];
        if (d->max_size > 32ull * ring || d->count > ring) return false;
        // room for the table at the larger of its limit, the default and the SETTINGS limit, within the ring
        size_t want = std::max<size_t>(d->max_size, 4096);
        if (d->has_max_allowed) want = std::max(want, d->max_allowed);
        const uint32_t cap = (uint32_t)std::min<size_t>(ring, std::max<size_t>((want + 31) / 32, d->count));
        x->tabs[k] = hpk_dtab{(uint32_t)x->ent.size(), cap, d->count, (uint32_t)d->size, (uint32_t)d->max_size,
                              d->has_max_allowed && d->max_allowed < HPK_DTAB_NO_LIMIT ? (uint32_t)d->max_allowed : HPK_DTAB_NO_LIMIT,
                              0u, 0u};
        const size_t e0 = x->ent.size();
        x->ent.resize(e0 + cap, hpk_header{0u, 0u, 0u, 0u});
        for (uint32_t i = 0; i < d->count; ++i) {
            const hpk_hdec::Ent& e = d->at(i);
            const uint32_t at = (uint32_t)(stext_len + x->prior.size());
            x->ent[e0 + i] = hpk_header{at, e.nl, at + e.nl, e.vl};
            x->prior.insert(x->prior.end(), d->bytes.data() + e.at, d->bytes.data() + e.at + e.nl + e.vl);
        }
    }
    return true;
}

// hpk_hdec_decode_blocks with HPK_BLOCK_APPLY_DEVICE (include/hpk.h has the steps): the blocks grouped by decoder,
// the tables out, the device pipeline with the apply kernel at its end, and either the finished headers and tables
// back, or (a block deferred) the device-scan path's host apply for the whole call. No decoder is written before
// everything is back.
int decode_blocks_apply_device(const Call& c) {
    const uint32_t nblocks = c.nblocks;
    if (nblocks == 0) return decode_blocks_device(c);
    const Timer t_0;
    uint32_t ring = 0, chunk = 0, wgd = 0;
    (void)hpk_test_blkapply_geometry(&ring, &chunk, &wgd);
    const hpk_groups<hpk_hdec> g = hpk_group_blocks(c.decs, nblocks);
    const uint32_t nd = (uint32_t)g.who.size();
    const uint8_t* stext = nullptr;
    size_t stext_len = 0;
    (void)hpk_static_table(&stext, &stext_len, nullptr);
    TablesOut x;
    bool fits = export_tables(g.who, ring, stext_len, &x);  // every table within the device ring
    const uint64_t str_base = (uint64_t)stext_len + x.prior.size();
    fits = fits && str_base + hpk_decoded_bound(c.block_off[nblocks]) + 16u < (1ull << 32) && x.ent.size() < (1ull << 32);
    if (!fits) return decode_blocks_device(c);
    hpk_applyplan plan{};
    plan.dec_blk_off = g.off.data();
    plan.dec_blk = g.list.data();
    plan.ndecs = nd;
    plan.tabs = x.tabs.data();
    plan.tab_ent = x.ent.data();
    plan.nent = (uint32_t)x.ent.size();
    plan.str_base = (uint32_t)str_base;
    const long us_export = t_0.us();
    hpk_blkdev h;
    if (int rc = hpk_blocks_device(c.ctx, c.blocks, c.block_off, nblocks, &h, &plan)) return rc;
    if (!plan.applied) return apply_blkdev_host(c, h);
    // everything is back: the outputs, then the decoders
    const Timer t_1;
    hpk_blocks_out* out = c.out;
    out->n_blocks = nblocks;
    out->arena_len = (size_t)str_base + plan.packed_len;
    out->n_headers = h.nfields;
    out->arena = (uint8_t*)g_out_cache.take(0, out->arena_len);
    out->headers = (hpk_header*)g_out_cache.take(1, (size_t)h.nfields * sizeof(hpk_header));
    out->blocks = (hpk_block_result*)g_out_cache.take(2, (size_t)nblocks * sizeof(hpk_block_result));
    if (!out->arena || !out->headers || !out->blocks) {
        hpk_blocks_out_free(out);
        return HPK_E_INVAL;
    }
    memcpy(out->arena, stext, stext_len);
    if (!x.prior.empty()) memcpy(out->arena + stext_len, x.prior.data(), x.prior.size());
    c.parallel([&](int t) {  // the packed bytes, the header records and the results, a slice per thread
        auto slice = [&](void* to, const void* from, size_t bytes) {
            const size_t lo = bytes * (size_t)t / (size_t)c.nth, hi = bytes * (size_t)(t + 1) / (size_t)c.nth;
            if (hi > lo) memcpy((uint8_t*)to + lo, (const uint8_t*)from + lo, hi - lo);
        };
        slice(out->arena + str_base, h.arena, plan.packed_len);
        slice(out->headers, plan.headers, (size_t)h.nfields * sizeof(hpk_header));
        slice(out->blocks, plan.results, (size_t)nblocks * sizeof(hpk_block_result));
    });
    for (uint32_t k = 0; k < nd; ++k) {  // each table from its final entries' bytes, oldest first
        hpk_hdec* d = g.who[k];
        const hpk_dtab& t = plan.tabs_out[k];
        d->clear();
        d->max_size = t.max_size;
        for (uint32_t i = t.count; i-- > 0;) {
            const hpk_header& e = plan.ent_out[t.ent + i];
            d->add(out->arena + e.name_off, e.name_len, out->arena + e.value_off, e.value_len);
        }
    }
    if (c.timing)
        fprintf(stderr,
                "hpk_hdec_decode_blocks: device apply, %u decoders, tables out %ld us, device scan %ld us, strings %ld us, "
                "apply and results back %ld us, outputs and tables in %ld us\n",
                nd, us_export, h.us_scan, h.us_strings - plan.us_apply, plan.us_apply, t_1.us());
    return HPK_E_OK;
}

// pass 1: scan every block, gather the Huffman strings (contiguous block ranges per thread)
void scan_blocks(BlockScratch& W, const Call& c, Batch* q) {
    const int nth = c.nth;
    W.scans.resize(c.nblocks);
    if ((int)W.pools.size() < nth) {
        W.pools.resize(nth);
        W.thoff.resize(nth);
        W.thlen.resize(nth);
    }
    q->ibase.assign(nth + 1, 0);
    q->obase.assign(nth + 1, 0);
    c.parallel([&](int t) {
        // the vectors are moved into locals while the thread appends: their headers sit next to
        // the other threads' in the scratch arrays (false sharing on every push_back otherwise)
        const size_t bytes = c.block_off[c.blk0(t + 1)] - c.block_off[c.blk0(t)];
        std::vector<Field> pool = std::move(W.pools[t]);
        std::vector<uint32_t> ho = std::move(W.thoff[t]), hl = std::move(W.thlen[t]);
        pool.clear();
        ho.clear();
        hl.clear();
        pool.reserve(bytes / 8 + 16);  // ~12 block bytes per field on the interop corpus
        ho.reserve(bytes / 8 + 16);
        hl.reserve(bytes / 8 + 16);
        for (uint32_t b = c.blk0(t); b < c.blk0(t + 1); ++b)
            scan_block(c.blocks, c.block_off[b], c.block_off[b + 1], (uint32_t)t, &pool, &W.scans[b], &ho, &hl);
        uint64_t ti = 0, to = 0;  // the thread's string bytes and their decoded bounds
        for (uint32_t x : hl) {
            ti += x;
            to += (hpk_decoded_bound(x) + 3) & ~(uint64_t)3;
        }
        q->ibase[t + 1] = ti;  // (summed below)
        q->obase[t + 1] = to;
        W.pools[t] = std::move(pool);
        W.thoff[t] = std::move(ho);
        W.thlen[t] = std::move(hl);
    });
    W.lbase.assign(nth + 1, 0);  // each thread's first index in the batch
    for (int t = 0; t < nth; ++t) {
        W.lbase[t + 1] = W.lbase[t] + (uint32_t)W.thoff[t].size();
        q->ibase[t + 1] += q->ibase[t];
        q->obase[t + 1] += q->obase[t];
    }
    q->n = W.lbase[nth];
    q->tot = q->ibase[nth];
    q->otot = q->obase[nth];
}

// pass 2: one batch for all of them, assembled and started. With a device context the batch is staged in the
// context's page-locked host area (hpk_ctx_pinned), so its copies are DMA transfers that overlap the kernel chunk by
// chunk; pageable vectors made HIP bounce every byte through its own staging buffer. Without one the CPU batch
// path decodes it here.
int stage_batch(BlockScratch& W, const Call& c, Batch* q) {
    const uint32_t n = q->n;
    if (q->tot >= (1ull << 32) || q->otot >= (1ull << 32)) return HPK_E_INVAL;
    const hpk_lay_hdecbatch& l = q->lay = hpk_layout_hdecbatch(q->tot, q->otot, n);
    if (c.ctx) {
        void* base = nullptr;
        if (int rc = hpk_ctx_pinned(c.ctx, l.bytes, &base)) return rc;
        q->in = l.in.in(base);
        q->dec = l.dec.in(base);
        q->in_off = l.in_off.in(base);
        q->out_off = l.out_off.in(base);
        q->len = l.len.in(base);
        q->st = l.st.in(base);
    } else {
        auto sized = [](auto& v, size_t count) { return v.resize(count), v.data(); };
        q->in = sized(W.in, l.in_cap());
        q->dec = sized(W.dec, l.dec_cap());
        q->in_off = sized(W.in_off, n + 1);
        q->out_off = sized(W.out_off, n + 1);
        q->len = sized(W.len, n ? n : 1);
        q->st = sized(W.st, n ? n : 1);
    }
    c.parallel([&](int t) {  // each thread's strings: offsets from its bases, bytes gathered
        uint64_t io = q->ibase[t], oo = q->obase[t];
        const uint32_t* ho = W.thoff[t].data();
        const uint32_t* hl = W.thlen[t].data();
        uint32_t* ino = q->in_off + W.lbase[t];
        uint32_t* ouo = q->out_off + W.lbase[t];
        for (size_t j = 0, m = W.thlen[t].size(); j < m; ++j) {
            ino[j] = (uint32_t)io;
            ouo[j] = (uint32_t)oo;
            memcpy(q->in + io, c.blocks + ho[j], hl[j]);
            io += hl[j];
            oo += (hpk_decoded_bound(hl[j]) + 3) & ~(uint64_t)3;
        }
    });
    q->in_off[n] = (uint32_t)q->tot;
    q->out_off[n] = (uint32_t)q->otot;
    q->cut.assign(c.ctx ? hpk_ctx_max_chunks() + 1 : 1, 0);
    if (!n) return HPK_E_OK;
    const int rc = c.ctx ? hpk_decode_host_begin(c.ctx, q->in, l.in_cap(), q->in_off, n, q->dec, l.dec_cap(), q->out_off, q->len,
                                                 q->st, &q->chunks, q->cut.data())
                         : hpk_decode_batch_cpu(q->in, q->in_off, n, q->dec, q->out_off, q->len, q->st, 0);
    if (rc && c.ctx && q->chunks) (void)hpk_decode_host_end(c.ctx);
    return rc;
}

// The default path's pass 3: the host scan's fields, the batch's results as they come back. A thread waits for
// chunk j's results only when it reaches a block with a string in it.
struct HostScanPath {
    const Call& c;
    const BlockScratch& W;
    const Batch& q;
    struct alignas(64) Waits {
        int waited = 0;  // device chunks whose results this thread has waited for
        int rc = 0;
    };
    std::vector<Waits> waits = std::vector<Waits>(c.nth);
    const Field* fields(uint32_t b) const { return W.pools[W.scans[b].pool].data() + W.scans[b].first; }
    uint64_t work(uint32_t b) const { return W.scans[b].n + 1u; }
    size_t headers(int t) const { return W.pools[t].size() + 16; }
    // a block's fields and its Huffman strings are fetched a few blocks ahead (a thread's blocks are scattered
    // over the batch: every string would otherwise be a cache miss on the critical path)
    void fetch_fields(uint32_t b) const {
        const Field* f = fields(b);
        for (uint32_t k = 0; k < W.scans[b].n; k += 1) __builtin_prefetch(f + k);
    }
    void fetch_strings(uint32_t b) const {
        const Field* f = fields(b);
        const uint32_t lb = W.lbase[W.scans[b].pool];
        for (uint32_t k = 0; k < W.scans[b].n; ++k) {
            if (f[k].name.huff) __builtin_prefetch(q.dec + q.out_off[lb + f[k].name.lit]);
            if (f[k].value.huff) __builtin_prefetch(q.dec + q.out_off[lb + f[k].value.lit]);
        }
    }
    int apply(int t, const uint32_t* my, size_t left, Out& o, hpk_block_result* res) {
        const uint32_t b = my[0];
        const Scan& sc = W.scans[b];
        Waits& w = waits[t];
        if (left > 4) fetch_fields(my[4]);
        if (left > 2) fetch_strings(my[2]);
        const uint32_t lb = W.lbase[sc.pool], lit_end = lb + sc.lit_end;  // the block's strings end
        while (w.waited < q.chunks && q.cut[w.waited] < lit_end)
            if ((w.rc = hpk_host_chunk_wait(c.ctx, w.waited++))) return w.rc;
        apply_block(c.decs[b], HostView{fields(b), sc.n, c.blocks, q, lb}, o, &res[b]);
        return 0;
    }
    int end() {
        int rc = q.chunks ? hpk_decode_host_end(c.ctx) : HPK_E_OK;
        for (int t = 0; t < c.nth && !rc; ++t) rc = waits[t].rc;
        return rc;
    }
};

}  // namespace

// Timeline of a call with a device context: scan (threads) -> the batch assembled in the pinned
// area (threads) -> the batch's chunks copied in, decoded and copied out on the device while the
// threads apply the blocks whose strings are back (a thread waits for chunk j's results only when
// it reaches a block with a string in it), so the device time hides under the apply pass.
extern "C" int hpk_hdec_decode_blocks(hpk_ctx* ctx, hpk_hdec* const* decs, const uint8_t* blocks,
                                      const uint32_t* block_off, uint32_t nblocks, hpk_blocks_out* out) {
    if (!decs || !block_off || !out || (nblocks && block_off[nblocks] && !blocks)) return HPK_E_INVAL;
    memset(out, 0, sizeof *out);
    for (uint32_t b = 0; b < nblocks; ++b)
        if (!decs[b] || block_off[b + 1] < block_off[b]) return HPK_E_INVAL;
    // Host threads: blocks are independent in pass 1; in pass 3 a decoder's blocks stay on one
    // thread, in order (apply_threaded).
    int nth = (int)std::thread::hardware_concurrency();
    if (const char* e = getenv("HPK_HDEC_THREADS")) nth = atoi(e);  // (for measurements)
    if (nth > Pool::kMax) nth = Pool::kMax;
    if (nth < 1) nth = 1;
    if ((uint32_t)nth > nblocks / 256u + 1u) nth = (int)(nblocks / 256u + 1u);
    static const bool timing = getenv("HPK_HDEC_TIMING") != nullptr;
    const Call c{ctx, decs, blocks, block_off, nblocks, out, nth,
                 [nth](const std::function<void(int)>& fn) { pool().run(nth, fn); }, timing};
    if (ctx && hpk_ctx_block_apply(ctx) == HPK_BLOCK_APPLY_DEVICE)  // opt-in: scan, strings and apply on the device
        return decode_blocks_apply_device(c);
    if (ctx && hpk_ctx_block_scan(ctx) == HPK_BLOCK_SCAN_DEVICE)  // opt-in: scan and strings on the device
        return decode_blocks_device(c);
    BlockScratch& W = t_scratch;
    Batch q;
    const Timer t_scan;
    scan_blocks(W, c, &q);
    const long us_scan = t_scan.us();
    const Timer t_batch;
    if (int rc = stage_batch(W, c, &q)) return rc;
    const long us_batch = t_batch.us();
    HostScanPath p{c, W, q};
    long us_apply = 0, us_join = 0;
    if (int rc = apply_threaded(p, c, &us_apply, &us_join)) return rc;
    if (timing)
        fprintf(stderr, "hpk_hdec_decode_blocks: %d threads, scan %ld us, batch %s %ld us, apply %ld us, join %ld us\n",
                nth, us_scan, ctx ? "issue" : "cpu", us_batch, us_apply, us_join);
    return HPK_E_OK;
}

extern "C" void hpk_blocks_out_free(hpk_blocks_out* out) {
    if (!out) return;
    g_out_cache.give(0, out->arena, out->arena_len);
    g_out_cache.give(1, out->headers, out->n_headers * sizeof(hpk_header));
    g_out_cache.give(2, out->blocks, (size_t)out->n_blocks * sizeof(hpk_block_result));
    memset(out, 0, sizeof *out);
}
