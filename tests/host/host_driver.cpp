// host_driver.cpp — a stand-alone program around the host codec of libhpk (hpk_cpu.cpp, hpk_hdec.cpp, hpk_henc.cpp, hpk_h2.cpp), for
// builds under a host sanitizer (tests/test_host_sanitizers.py builds it plain, with ASan + UBSan and with TSan, each
// time together with the host units and tests/host/device_stubs.cpp; libhpk.so is not linked).
//
//   host_driver CASEFILE
//
// The case file (written by tests/host_cases.py; little-endian u32 words, `bytes` = a u32 length and that many octets)
// holds inputs AND expected results, the latter from oracle/hpack_ref.py and the C oracle, never from the library. It
// is the u32 magic 'HPKC' and then sections, each a u32 tag and a body, up to tag 0:
//   1 decode   decoders (optional set_max_table_size, blocks that prime the table, optional set_max_allowed_table_size),
//              calls of hpk_hdec_decode_blocks(NULL, ...) as lists of (decoder, block) with, per block, n_headers,
//              error, detail and the headers' bytes; per decoder the table sizes after the last call;
//   2 encode   encoders (Huffman on or off, optional set_max_table_size), calls through hpk_henc_encode (kind 0; kind 2:
//              first with cap one below the need: HPK_E_NOSPACE, the need in *out_len, the state unchanged) and through
//              hpk_henc_encode_blocks(NULL, ...) (kind 1; kind 3: first with hpk_test_fail_batches(1): HPK_E_DEVICE, the
//              tables untouched, then the same call again), with the block bytes; per encoder the table sizes;
//   3 h2       connections (optional set_max_frame_size), calls of hpk_h2_read_frames(NULL, ...) with conn_error,
//              conn_consumed, the hpk_h2_block records and the decoded headers; per connection its error at the end;
//   4 huffman  hpk_huffman_decode_one / _encode_one at exact capacity and one below, hpk_decode_batch_cpu and
//              hpk_encode_batch_cpu over all of them with 1 and with 4 threads, regions of exact capacity back to back;
//   5 threads  N callers start together (a barrier, again before every round), each with its own decoders or encoders,
//              and replay the decode or encode section that follows R times;
//   6 fork     the decode section that follows runs in the parent (its pooled calls start the pool's threads), the
//              parent forks, the child runs it again and _exit()s with 0 or 1, the parent waits and checks the status.
// Every input handed to the library is an exact-size heap copy (malloc(n): a call's block blob, its offsets, the frame
// bytes, the field blob, a literal), and single-literal outputs are exact-size too: a read or write one byte past
// any of them is an AddressSanitizer report.
// Output: the first mismatches, the counts the test asserts coverage on (block errors, Huffman details, connection
// errors, the threaded mode's big calls and overlap), and `ok: 0 mismatches in N cases` (exit status 0) or `FAIL: ...`.
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/wait.h>
#include <unistd.h>

#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hpk.h"

namespace {

typedef std::vector<uint8_t> Bytes;

std::atomic<long> g_cases{0}, g_bad{0};
std::atomic<long> g_blk_err[16], g_huff_detail[8], g_h2_err[16], g_lit_status[8];
std::atomic<int> g_in_call{0}, g_max_overlap{0};
std::atomic<long> g_big_calls{0};

void mismatch(const std::string& what) {
    if (g_bad.fetch_add(1) < 10) fprintf(stdout, "mismatch: %s\n", what.c_str());
}
#define CHECK(cond, ...)                              \
    do {                                              \
        if (!(cond)) {                                \
            char b_[256];                             \
            snprintf(b_, sizeof b_, __VA_ARGS__);     \
            mismatch(b_);                             \
        }                                             \
    } while (0)

// an exact-size heap copy: malloc(n), n == 0 included (a zero-size region: any access to it is a report)
template <class T>
struct Exact {
    T* p;
    explicit Exact(size_t n) : p((T*)malloc(n * sizeof(T))) {
        if (!p) abort();
    }
    Exact(const T* src, size_t n) : Exact(n) {
        if (n) memcpy(p, src, n * sizeof(T));
    }
    ~Exact() { free(p); }
    Exact(const Exact&) = delete;
    Exact& operator=(const Exact&) = delete;
};

struct Reader {
    const uint8_t* p;
    const uint8_t* end;
    uint32_t u32() {
        if (end - p < 4) {
            fprintf(stderr, "case file: truncated\n");
            exit(2);
        }
        uint32_t v;
        memcpy(&v, p, 4);
        p += 4;
        return v;
    }
    int32_t i32() { return (int32_t)u32(); }
    Bytes bytes() {
        const uint32_t n = u32();
        if ((size_t)(end - p) < n) {
            fprintf(stderr, "case file: truncated\n");
            exit(2);
        }
        Bytes b(p, p + n);
        p += n;
        return b;
    }
};

struct Header {
    Bytes name, value;
};
std::vector<Header> read_headers(Reader& r, uint32_t n) {
    std::vector<Header> h(n);
    for (auto& x : h) {
        x.name = r.bytes();
        x.value = r.bytes();
    }
    return h;
}

// headers [first, first + n) of a blocks_out against the expected list
void check_headers(const hpk_blocks_out& o, const hpk_block_result& res, const std::vector<Header>& want, const char* where,
                   size_t idx) {
    if (res.n_headers != want.size()) return;  // (reported by the caller)
    for (size_t j = 0; j < want.size(); ++j) {
        if ((size_t)res.first_header + j >= o.n_headers) {
            CHECK(false, "%s %zu: header %zu outside the header array", where, idx, j);
            return;
        }
        const hpk_header& h = o.headers[res.first_header + j];
        const bool in = (size_t)h.name_off + h.name_len <= o.arena_len && (size_t)h.value_off + h.value_len <= o.arena_len;
        CHECK(in, "%s %zu: header %zu outside the arena", where, idx, j);
        if (!in) return;
        const bool same = h.name_len == want[j].name.size() && h.value_len == want[j].value.size() &&
                          (h.name_len == 0 || !memcmp(o.arena + h.name_off, want[j].name.data(), h.name_len)) &&
                          (h.value_len == 0 || !memcmp(o.arena + h.value_off, want[j].value.data(), h.value_len));
        CHECK(same, "%s %zu: header %zu differs", where, idx, j);
        if (!same) return;
    }
}

void count_block_error(int error, int detail) {
    if (error >= 0 && error < 16) g_blk_err[error]++;
    if (error == HPK_BLK_STR_HUFFMAN && detail >= 0 && detail < 8) g_huff_detail[detail]++;
}

// ---- decode ----------------------------------------------------------------------------------------------------
struct DecSpec {
    uint32_t has_max, max_size, has_allowed, max_allowed;
    std::vector<Bytes> prime;
    uint32_t size, entries, end_max;
};
struct DecBlock {
    uint32_t dec;
    Bytes wire;
    uint32_t n_headers;
    int32_t error, detail;
    std::vector<Header> headers;
};
struct DecodeSection {
    std::vector<DecSpec> decs;
    std::vector<std::vector<DecBlock>> calls;
};

DecodeSection read_decode(Reader& r) {
    DecodeSection s;
    s.decs.resize(r.u32());
    for (auto& d : s.decs) {
        d.has_max = r.u32();
        d.max_size = r.u32();
        d.has_allowed = r.u32();
        d.max_allowed = r.u32();
        d.prime.resize(r.u32());
        for (auto& b : d.prime) b = r.bytes();
    }
    s.calls.resize(r.u32());
    for (auto& c : s.calls) {
        c.resize(r.u32());
        for (auto& b : c) {
            b.dec = r.u32();
            b.wire = r.bytes();
            b.n_headers = r.u32();
            b.error = r.i32();
            b.detail = r.i32();
            b.headers = read_headers(r, b.n_headers);
        }
    }
    for (auto& d : s.decs) {
        d.size = r.u32();
        d.entries = r.u32();
        d.end_max = r.u32();
    }
    return s;
}

// one hpk_hdec_decode_blocks(NULL, ...) over exact-size copies; returns its status
int decode_call(const std::vector<hpk_hdec*>& decs, const std::vector<const Bytes*>& wires, hpk_blocks_out* out) {
    const uint32_t n = (uint32_t)wires.size();
    size_t total = 0;
    for (auto* w : wires) total += w->size();
    Exact<uint8_t> blob(total);
    Exact<uint32_t> off((size_t)n + 1);
    Exact<hpk_hdec*> dp(decs.data(), n);
    size_t at = 0;
    for (uint32_t b = 0; b < n; ++b) {
        off.p[b] = (uint32_t)at;
        if (!wires[b]->empty()) memcpy(blob.p + at, wires[b]->data(), wires[b]->size());
        at += wires[b]->size();
    }
    off.p[n] = (uint32_t)at;
    const int now = ++g_in_call;
    int seen = g_max_overlap.load();
    while (now > seen && !g_max_overlap.compare_exchange_weak(seen, now)) {
    }
    if (n >= 1024) g_big_calls++;
    const int rc = hpk_hdec_decode_blocks(nullptr, dp.p, blob.p, off.p, n, out);
    --g_in_call;
    return rc;
}

void run_decode(const DecodeSection& s) {
    std::vector<hpk_hdec*> decs(s.decs.size());
    for (size_t k = 0; k < decs.size(); ++k) {
        const DecSpec& d = s.decs[k];
        decs[k] = hpk_hdec_create();
        if (!decs[k]) abort();
        if (d.has_max) CHECK(hpk_hdec_set_max_table_size(decs[k], d.max_size) == HPK_E_OK, "decoder %zu: set_max_table_size", k);
        for (const Bytes& w : d.prime) {
            hpk_blocks_out o = {};
            const int rc = decode_call({decs[k]}, {&w}, &o);
            CHECK(rc == HPK_E_OK && o.n_blocks == 1 && o.blocks[0].error == HPK_BLK_OK, "decoder %zu: priming block failed", k);
            hpk_blocks_out_free(&o);
        }
        if (d.has_allowed)
            CHECK(hpk_hdec_set_max_allowed_table_size(decs[k], d.max_allowed) == HPK_E_OK, "decoder %zu: set_max_allowed", k);
    }
    for (size_t c = 0; c < s.calls.size(); ++c) {
        const auto& call = s.calls[c];
        std::vector<hpk_hdec*> dd;
        std::vector<const Bytes*> ww;
        for (const DecBlock& b : call) {
            dd.push_back(decs[b.dec]);
            ww.push_back(&b.wire);
        }
        hpk_blocks_out o = {};
        const int rc = decode_call(dd, ww, &o);
        CHECK(rc == HPK_E_OK && o.n_blocks == call.size(), "decode call %zu: status %d, %u blocks", c, rc, o.n_blocks);
        for (size_t b = 0; b < call.size(); ++b) {
            g_cases++;
            if (rc != HPK_E_OK || o.n_blocks != call.size()) continue;
            const hpk_block_result& res = o.blocks[b];
            const DecBlock& w = call[b];
            CHECK(res.n_headers == w.n_headers && res.error == w.error && res.detail == w.detail,
                  "decode call %zu block %zu: %u headers, error %d detail %d for %u, %d, %d", c, b, res.n_headers, res.error,
                  res.detail, w.n_headers, w.error, w.detail);
            check_headers(o, res, w.headers, "decode block", b);
            count_block_error(w.error, w.detail);
        }
        hpk_blocks_out_free(&o);
    }
    for (size_t k = 0; k < decs.size(); ++k) {
        size_t size = 0, entries = 0, mx = 0;
        hpk_hdec_table_size(decs[k], &size, &entries, &mx);
        g_cases++;
        CHECK(size == s.decs[k].size && entries == s.decs[k].entries && mx == s.decs[k].end_max,
              "decoder %zu: table %zu octets, %zu entries, max %zu for %u, %u, %u", k, size, entries, mx, s.decs[k].size,
              s.decs[k].entries, s.decs[k].end_max);
        hpk_hdec_destroy(decs[k]);
    }
}

// ---- encode ----------------------------------------------------------------------------------------------------
struct EncSpec {
    uint32_t huffman, has_max, max_size;
    uint32_t size, entries, end_max;
};
struct EncBlock {
    uint32_t enc;
    std::vector<Header> headers;
    Bytes want;
};
struct EncCall {
    uint32_t kind;
    std::vector<EncBlock> blocks;
};
struct EncodeSection {
    std::vector<EncSpec> encs;
    std::vector<EncCall> calls;
};

EncodeSection read_encode(Reader& r) {
    EncodeSection s;
    s.encs.resize(r.u32());
    for (auto& e : s.encs) {
        e.huffman = r.u32();
        e.has_max = r.u32();
        e.max_size = r.u32();
    }
    s.calls.resize(r.u32());
    for (auto& c : s.calls) {
        c.kind = r.u32();
        c.blocks.resize(r.u32());
        for (auto& b : c.blocks) {
            b.enc = r.u32();
            b.headers = read_headers(r, r.u32());
            b.want = r.bytes();
        }
    }
    for (auto& e : s.encs) {
        e.size = r.u32();
        e.entries = r.u32();
        e.end_max = r.u32();
    }
    return s;
}

struct TableSize {
    size_t size, entries, max_size;
    bool operator==(const TableSize& o) const { return size == o.size && entries == o.entries && max_size == o.max_size; }
};
TableSize enc_size(const hpk_henc* e) {
    TableSize t{};
    hpk_henc_table_size(e, &t.size, &t.entries, &t.max_size);
    return t;
}

void run_encode(const EncodeSection& s) {
    std::vector<hpk_henc*> encs(s.encs.size());
    for (size_t k = 0; k < encs.size(); ++k) {
        encs[k] = hpk_henc_create((int)s.encs[k].huffman);
        if (!encs[k]) abort();
        if (s.encs[k].has_max) CHECK(hpk_henc_set_max_table_size(encs[k], s.encs[k].max_size) == HPK_E_OK, "encoder %zu: set_max", k);
    }
    for (size_t c = 0; c < s.calls.size(); ++c) {
        const EncCall& call = s.calls[c];
        // the fields end to end, header j's name then its value (hpk_henc_encode's layout), exact size
        size_t nh = 0, nbytes = 0;
        for (const auto& b : call.blocks)
            for (const auto& h : b.headers) nh += 1, nbytes += h.name.size() + h.value.size();
        Exact<uint8_t> fields(nbytes);
        Exact<uint32_t> foff(2 * nh + 1), hoff(call.blocks.size() + 1);
        Exact<hpk_henc*> ep(call.blocks.size());
        size_t at = 0, j = 0;
        for (size_t b = 0; b < call.blocks.size(); ++b) {
            hoff.p[b] = (uint32_t)j;
            ep.p[b] = encs[call.blocks[b].enc];
            for (const auto& h : call.blocks[b].headers) {
                foff.p[2 * j] = (uint32_t)at;
                if (!h.name.empty()) memcpy(fields.p + at, h.name.data(), h.name.size());
                at += h.name.size();
                foff.p[2 * j + 1] = (uint32_t)at;
                if (!h.value.empty()) memcpy(fields.p + at, h.value.data(), h.value.size());
                at += h.value.size();
                ++j;
            }
        }
        hoff.p[call.blocks.size()] = (uint32_t)j;
        foff.p[2 * nh] = (uint32_t)at;
        std::vector<TableSize> before;
        for (const auto& b : call.blocks) before.push_back(enc_size(encs[b.enc]));
        auto unchanged = [&] {
            for (size_t b = 0; b < call.blocks.size(); ++b)
                if (!(enc_size(encs[call.blocks[b].enc]) == before[b])) return false;
            return true;
        };
        if (call.kind == 0 || call.kind == 2) {  // hpk_henc_encode, one block
            const EncBlock& b = call.blocks[0];
            const size_t need = b.want.size();
            g_cases++;
            if (call.kind == 2 && need > 0) {
                Exact<uint8_t> small(need - 1);
                size_t got = 0;
                const int rc = hpk_henc_encode(ep.p[0], fields.p, foff.p, nh, small.p, need - 1, &got);
                CHECK(rc == HPK_E_NOSPACE && got == need, "encode call %zu: cap one below: status %d, need %zu for %zu", c, rc, got, need);
                CHECK(unchanged(), "encode call %zu: HPK_E_NOSPACE changed the encoder's table", c);
            }
            Exact<uint8_t> out(need);
            size_t got = 0;
            const int rc = hpk_henc_encode(ep.p[0], fields.p, foff.p, nh, out.p, need, &got);
            CHECK(rc == HPK_E_OK && got == need && (need == 0 || !memcmp(out.p, b.want.data(), need)),
                  "encode call %zu: hpk_henc_encode: status %d, %zu bytes for %zu", c, rc, got, need);
            continue;
        }
        if (call.kind == 3) {  // an injected failure of the Huffman batch: every table as it was
            hpk_test_fail_batches(1);
            hpk_henc_out o = {};
            const int rc = hpk_henc_encode_blocks(nullptr, ep.p, fields.p, foff.p, hoff.p, (uint32_t)call.blocks.size(), &o);
            hpk_test_fail_batches(0);
            CHECK(rc == HPK_E_DEVICE && o.bytes == nullptr && o.block_off == nullptr, "encode call %zu: injected failure: status %d", c, rc);
            CHECK(unchanged(), "encode call %zu: a failed hpk_henc_encode_blocks changed a table", c);
            hpk_henc_out_free(&o);
        }
        hpk_henc_out o = {};
        const int now = ++g_in_call;
        int seen = g_max_overlap.load();
        while (now > seen && !g_max_overlap.compare_exchange_weak(seen, now)) {
        }
        if (call.blocks.size() >= 1024) g_big_calls++;
        const int rc = hpk_henc_encode_blocks(nullptr, ep.p, fields.p, foff.p, hoff.p, (uint32_t)call.blocks.size(), &o);
        --g_in_call;
        CHECK(rc == HPK_E_OK && o.n_blocks == call.blocks.size(), "encode call %zu: status %d, %u blocks", c, rc, o.n_blocks);
        for (size_t b = 0; b < call.blocks.size(); ++b) {
            g_cases++;
            if (rc != HPK_E_OK || o.n_blocks != call.blocks.size()) continue;
            const Bytes& w = call.blocks[b].want;
            const size_t lo = o.block_off[b], hi = o.block_off[b + 1];
            CHECK(hi >= lo && hi <= o.len && hi - lo == w.size() && (w.empty() || !memcmp(o.bytes + lo, w.data(), w.size())),
                  "encode call %zu block %zu: %zu bytes for %zu", c, b, hi - lo, w.size());
        }
        hpk_henc_out_free(&o);
    }
    for (size_t k = 0; k < encs.size(); ++k) {
        const TableSize t = enc_size(encs[k]);
        g_cases++;
        CHECK(t.size == s.encs[k].size && t.entries == s.encs[k].entries && t.max_size == s.encs[k].end_max,
              "encoder %zu: table %zu octets, %zu entries, max %zu for %u, %u, %u", k, t.size, t.entries, t.max_size, s.encs[k].size,
              s.encs[k].entries, s.encs[k].end_max);
        hpk_henc_destroy(encs[k]);
    }
}

// ---- h2 --------------------------------------------------------------------------------------------------------
void run_h2(Reader& r) {
    std::vector<hpk_h2conn*> conns(r.u32());
    for (size_t k = 0; k < conns.size(); ++k) {
        conns[k] = hpk_h2conn_create();
        if (!conns[k]) abort();
        if (const uint32_t mf = r.u32()) CHECK(hpk_h2conn_set_max_frame_size(conns[k], mf) == HPK_E_OK, "connection %zu: set_max_frame_size", k);
    }
    const uint32_t ncalls = r.u32();
    for (uint32_t c = 0; c < ncalls; ++c) {
        const uint32_t n = r.u32();
        std::vector<hpk_h2conn*> cc(n);
        std::vector<Bytes> chunks(n);
        std::vector<int32_t> werr(n);
        std::vector<uint32_t> wcons(n);
        size_t total = 0;
        for (uint32_t k = 0; k < n; ++k) {
            cc[k] = conns[r.u32()];
            chunks[k] = r.bytes();
            werr[k] = r.i32();
            wcons[k] = r.u32();
            total += chunks[k].size();
        }
        Exact<uint8_t> bytes(total);
        Exact<uint32_t> off((size_t)n + 1);
        Exact<hpk_h2conn*> cp(cc.data(), n);
        size_t at = 0;
        for (uint32_t k = 0; k < n; ++k) {
            off.p[k] = (uint32_t)at;
            if (!chunks[k].empty()) memcpy(bytes.p + at, chunks[k].data(), chunks[k].size());
            at += chunks[k].size();
        }
        off.p[n] = (uint32_t)at;
        hpk_h2_out o = {};
        const int rc = hpk_h2_read_frames(nullptr, cp.p, bytes.p, off.p, n, &o);
        CHECK(rc == HPK_E_OK && o.n_conns == n, "h2 call %u: status %d", c, rc);
        const bool ok = rc == HPK_E_OK && o.n_conns == n;
        for (uint32_t k = 0; k < n; ++k) {
            g_cases++;
            if (werr[k] >= 0 && werr[k] < 16) g_h2_err[werr[k]]++;
            if (!ok) continue;
            CHECK(o.conn_error[k] == werr[k] && o.conn_consumed[k] == wcons[k], "h2 call %u connection %u: error %d consumed %u for %d, %u",
                  c, k, o.conn_error[k], o.conn_consumed[k], werr[k], wcons[k]);
        }
        const uint32_t nb = r.u32();
        CHECK(!ok || o.hb.n_blocks == nb, "h2 call %u: %u blocks for %u", c, ok ? o.hb.n_blocks : 0u, nb);
        for (uint32_t b = 0; b < nb; ++b) {
            const uint32_t conn = r.u32(), stream = r.u32(), es = r.u32(), skipped = r.u32(), nh = r.u32();
            const int32_t error = r.i32(), detail = r.i32();
            const std::vector<Header> want = read_headers(r, nh);
            g_cases++;
            if (!ok || o.hb.n_blocks != nb) continue;
            const hpk_h2_block& m = o.blocks[b];
            CHECK(m.conn == conn && m.stream_id == stream && m.end_stream == es && m.skipped == skipped,
                  "h2 call %u block %u: conn %u stream %u end_stream %u skipped %u for %u, %u, %u, %u", c, b, m.conn, m.stream_id,
                  m.end_stream, m.skipped, conn, stream, es, skipped);
            if (skipped) continue;  // (not decoded by the reference: nothing to compare)
            const hpk_block_result& res = o.hb.blocks[b];
            CHECK(res.n_headers == nh && res.error == error && res.detail == detail, "h2 call %u block %u: %u headers, error %d detail %d for %u, %d, %d",
                  c, b, res.n_headers, res.error, res.detail, nh, error, detail);
            check_headers(o.hb, res, want, "h2 block", b);
            count_block_error(error, detail);
        }
        hpk_h2_out_free(&o);
    }
    for (size_t k = 0; k < conns.size(); ++k) {
        const int32_t want = r.i32();
        g_cases++;
        CHECK(hpk_h2conn_error(conns[k]) == want, "connection %zu: error %d for %d at the end", k, hpk_h2conn_error(conns[k]), want);
        hpk_h2conn_destroy(conns[k]);
    }
}

// ---- huffman ---------------------------------------------------------------------------------------------------
struct Lit {
    Bytes in, out, out_m1;  // decode: out at the bound's capacity, out_m1 at len(out) - 1; encode: out the encoding
    int32_t status, status_m1;
};

template <bool kEncode>
void run_batch(const std::vector<Lit>& lits, int nthreads) {
    const uint32_t n = (uint32_t)lits.size();
    size_t ti = 0, to = 0;
    for (const Lit& l : lits) ti += l.in.size(), to += l.out.size();
    Exact<uint8_t> in(ti), out(to), st(n);
    Exact<uint32_t> ioff((size_t)n + 1), ooff((size_t)n + 1), olen(n);
    size_t a = 0, b = 0;
    for (uint32_t i = 0; i < n; ++i) {
        ioff.p[i] = (uint32_t)a;
        ooff.p[i] = (uint32_t)b;
        if (!lits[i].in.empty()) memcpy(in.p + a, lits[i].in.data(), lits[i].in.size());
        a += lits[i].in.size();
        b += lits[i].out.size();
    }
    ioff.p[n] = (uint32_t)a;
    ooff.p[n] = (uint32_t)b;
    const int rc = kEncode ? hpk_encode_batch_cpu(in.p, ioff.p, n, out.p, ooff.p, olen.p, st.p, nthreads)
                           : hpk_decode_batch_cpu(in.p, ioff.p, n, out.p, ooff.p, olen.p, st.p, nthreads);
    CHECK(rc == HPK_E_OK, "%s batch on %d threads: status %d", kEncode ? "encode" : "decode", nthreads, rc);
    if (rc != HPK_E_OK) return;
    for (uint32_t i = 0; i < n; ++i) {
        const Lit& l = lits[i];
        const int want = kEncode ? HPK_OK : l.status;
        CHECK(st.p[i] == want && olen.p[i] == l.out.size() && (l.out.empty() || !memcmp(out.p + ooff.p[i], l.out.data(), l.out.size())),
              "%s batch on %d threads, literal %u: status %d, %u bytes for %d, %zu", kEncode ? "encode" : "decode", nthreads, i, st.p[i],
              olen.p[i], want, l.out.size());
    }
}

void run_huffman(Reader& r) {
    std::vector<Lit> dec(r.u32());
    for (Lit& l : dec) {
        l.in = r.bytes();
        l.status = r.i32();
        l.out = r.bytes();
        l.status_m1 = r.i32();
        l.out_m1 = r.bytes();
    }
    for (size_t i = 0; i < dec.size(); ++i) {
        const Lit& l = dec[i];
        g_cases++;
        if (l.status >= 0 && l.status < 8) g_lit_status[l.status]++;
        Exact<uint8_t> in(l.in.data(), l.in.size());
        {
            Exact<uint8_t> out(l.out.size());
            size_t got = 0;
            const int st = hpk_huffman_decode_one(in.p, l.in.size(), out.p, l.out.size(), &got);
            CHECK(st == l.status && got == l.out.size() && (got == 0 || !memcmp(out.p, l.out.data(), got)),
                  "decode_one %zu at exact capacity: status %d, %zu bytes for %d, %zu", i, st, got, l.status, l.out.size());
        }
        if (!l.out.empty()) {
            const size_t cap = l.out.size() - 1;
            Exact<uint8_t> out(cap);
            size_t got = 0;
            const int st = hpk_huffman_decode_one(in.p, l.in.size(), out.p, cap, &got);
            CHECK(st == l.status_m1 && got == l.out_m1.size() && (got == 0 || !memcmp(out.p, l.out_m1.data(), got)),
                  "decode_one %zu one below: status %d, %zu bytes for %d, %zu", i, st, got, l.status_m1, l.out_m1.size());
        }
    }
    std::vector<Lit> enc(r.u32());
    for (Lit& l : enc) {
        l.in = r.bytes();
        l.out = r.bytes();
        l.status = 0;
    }
    for (size_t i = 0; i < enc.size(); ++i) {
        const Lit& l = enc[i];
        g_cases++;
        Exact<uint8_t> in(l.in.data(), l.in.size());
        CHECK(hpk_huffman_encoded_len(in.p, l.in.size()) == l.out.size(), "encoded_len %zu", i);
        {
            Exact<uint8_t> out(l.out.size());
            size_t got = 0;
            const int st = hpk_huffman_encode_one(in.p, l.in.size(), out.p, l.out.size(), &got);
            CHECK(st == HPK_E_OK && got == l.out.size() && (got == 0 || !memcmp(out.p, l.out.data(), got)),
                  "encode_one %zu at exact capacity: status %d, %zu bytes for %zu", i, st, got, l.out.size());
        }
        if (!l.out.empty()) {  // one below: HPK_E_NOSPACE, the encoding's first cap bytes
            const size_t cap = l.out.size() - 1;
            Exact<uint8_t> out(cap);
            size_t got = 0;
            const int st = hpk_huffman_encode_one(in.p, l.in.size(), out.p, cap, &got);
            CHECK(st == HPK_E_NOSPACE && got == cap && (cap == 0 || !memcmp(out.p, l.out.data(), cap)),
                  "encode_one %zu one below: status %d, %zu bytes for cap %zu", i, st, got, cap);
        }
    }
    for (int nth : {1, 4}) {
        run_batch<false>(dec, nth);
        run_batch<true>(enc, nth);
    }
}

// ---- threads and fork ----------------------------------------------------------------------------------------
void run_threads(Reader& r) {
    const uint32_t n = r.u32(), rounds = r.u32(), kind = r.u32();
    DecodeSection ds;
    EncodeSection es;
    if (kind == 1)
        ds = read_decode(r);
    else
        es = read_encode(r);
    g_max_overlap = 0;  // (the overlap this section's callers reach)
    pthread_barrier_t bar;
    pthread_barrier_init(&bar, nullptr, n);
    std::vector<std::thread> th;
    for (uint32_t t = 0; t < n; ++t)
        th.emplace_back([&] {
            for (uint32_t k = 0; k < rounds; ++k) {
                pthread_barrier_wait(&bar);  // the callers enter every round together
                if (kind == 1)
                    run_decode(ds);
                else
                    run_encode(es);
            }
        });
    for (auto& x : th) x.join();
    pthread_barrier_destroy(&bar);
    printf("threads: %u callers, %u rounds, kind %u, %ld calls of >= 1024 blocks so far, max overlap %d\n", n, rounds, kind, g_big_calls.load(),
           g_max_overlap.load());
}

void run_fork(Reader& r) {
    const DecodeSection ds = read_decode(r);
    run_decode(ds);  // (the parent's pooled calls: the pool's threads exist now)
    fflush(stdout);
    fflush(stderr);
    const long bad_before = g_bad.load();
    const pid_t pid = fork();
    if (pid < 0) {
        mismatch("fork failed");
        return;
    }
    if (pid == 0) {  // the child: the same calls on fresh decoders; its pool must be a fresh one
        run_decode(ds);
        fflush(stdout);
        _exit(g_bad.load() == bad_before ? 0 : 1);
    }
    int status = 0;
    const pid_t got = waitpid(pid, &status, 0);
    g_cases++;
    CHECK(got == pid && WIFEXITED(status) && WEXITSTATUS(status) == 0, "fork: the child's status is 0x%x", status);
    run_decode(ds);  // the parent's pool still works
    printf("fork: child exit status %d\n", WIFEXITED(status) ? WEXITSTATUS(status) : -1);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: host_driver CASEFILE\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    Bytes file;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + k);
    fclose(f);
    Reader r{file.data(), file.data() + file.size()};
    if (r.u32() != 0x434B5048u) {
        fprintf(stderr, "%s: not a case file\n", argv[1]);
        return 2;
    }
    for (;;) {
        const uint32_t tag = r.u32();
        if (tag == 0) break;
        if (tag == 1)
            run_decode(read_decode(r));
        else if (tag == 2)
            run_encode(read_encode(r));
        else if (tag == 3)
            run_h2(r);
        else if (tag == 4)
            run_huffman(r);
        else if (tag == 5)
            run_threads(r);
        else if (tag == 6)
            run_fork(r);
        else {
            fprintf(stderr, "%s: unknown section %u\n", argv[1], tag);
            return 2;
        }
    }
    for (int e = 0; e < 16; ++e)
        if (g_blk_err[e].load()) printf("blk_error %d: %ld\n", e, g_blk_err[e].load());
    for (int e = 0; e < 8; ++e)
        if (g_huff_detail[e].load()) printf("huff_detail %d: %ld\n", e, g_huff_detail[e].load());
    for (int e = 0; e < 8; ++e)
        if (g_lit_status[e].load()) printf("lit_status %d: %ld\n", e, g_lit_status[e].load());
    for (int e = 0; e < 16; ++e)
        if (g_h2_err[e].load()) printf("h2_error %d: %ld\n", e, g_h2_err[e].load());
    const long bad = g_bad.load();
    if (bad)
        printf("FAIL: %ld mismatches in %ld cases\n", bad, g_cases.load());
    else
        printf("ok: 0 mismatches in %ld cases\n", g_cases.load());
    return bad != 0;
}
