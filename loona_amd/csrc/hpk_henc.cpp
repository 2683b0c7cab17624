// hpk_henc.cpp — the HPACK header-block encoder (the response path). Host code: the C ABI's hpk_henc_* entry
// points (include/hpk.h).
//
// Reference: hpack::Encoder, crates/loona-hpack/src/encoder.rs:172-335, with
// the H-bit rule as an option. The dynamic table is the reference's (lib.rs:43-164; the same
// eviction as hpk_hdec), the lookup its find_header (lib.rs:261-288): static then dynamic
// (newest first), the first full match, else the LAST name match.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <string>
#include <vector>

#include "../../include/hpk.h"
#include "hpk_hpack.h"
#include "hpk_internal.h"  // the context's calls that are not in the C ABI: the device-plan path

int hpk_set_err_msg(const char* what, int code);  // hpk_ctx.hip: hpk_last_error's message

namespace {
// The three representations the reference's encoder uses (encoder.rs:210-234)
enum Form { kLiteral, kIndexedName, kIndexed };
struct Rep {
    Form form;
    size_t index;  // 1-based; kLiteral has none
};
}  // namespace

struct hpk_henc {
    std::deque<std::pair<std::string, std::string>> table;  // front = newest
    size_t size = 0;
    size_t max_size = 4096;
    int huffman = 0;

    void consolidate() {
        while (size > max_size) {
            const auto& last = table.back();
            size -= last.first.size() + last.second.size() + 32;
            table.pop_back();
        }
    }
    void add(std::string n, std::string v) {
        size += n.size() + v.size() + 32;
        table.emplace_front(std::move(n), std::move(v));
        consolidate();
    }
    // 1-based index, 0 = no name match; *full = name and value matched
    size_t find(const uint8_t* n, size_t nl, const uint8_t* v, size_t vl, bool* full) const {
        size_t name_match = 0;
        for (size_t i = 0; i < 61; ++i) {
            const std::string_view sn = hpk_static[i][0], sv = hpk_static[i][1];
            if (sn.size() == nl && !memcmp(sn.data(), n, nl)) {
                if (sv.size() == vl && !memcmp(sv.data(), v, vl)) {
                    *full = true;
                    return i + 1;
                }
                name_match = i + 1;
            }
        }
        for (size_t j = 0; j < table.size(); ++j) {
            const auto& e = table[j];
            if (e.first.size() == nl && !memcmp(e.first.data(), n, nl)) {
                if (e.second.size() == vl && !memcmp(e.second.data(), v, vl)) {
                    *full = true;
                    return 62 + j;
                }
                name_match = 62 + j;
            }
        }
        *full = false;
        return name_match;
    }
    // One header's representation, the table updated for it: indexed (encoder.rs:329-334); indexed name, the value
    // not indexed (encoder.rs:311-323); or a literal with incremental indexing (encoder.rs:279-291) and add_header.
    Rep choose(const uint8_t* n, size_t nl, const uint8_t* v, size_t vl) {
        bool full = false;
        const size_t idx = find(n, nl, v, vl, &full);
        if (idx) return Rep{full ? kIndexed : kIndexedName, idx};
        add(std::string((const char*)n, nl), std::string((const char*)v, vl));
        return Rep{kLiteral, 0};
    }
};

namespace {

// encode_integer_into (encoder.rs:93-122)
void put_integer(std::vector<uint8_t>& o, size_t value, int prefix, uint8_t leading) {
    const size_t mask = prefix >= 8 ? 0xFFu : ((1u << prefix) - 1u);
    leading &= (uint8_t)~mask;
    if (value < mask) {
        o.push_back((uint8_t)(leading | value));
        return;
    }
    o.push_back((uint8_t)(leading | mask));
    value -= mask;
    while (value >= 128) {
        o.push_back((uint8_t)(value % 128 + 128));
        value /= 128;
    }
    o.push_back((uint8_t)value);
}

// a representation's octets in front of its string literals (a literal's name and value; an indexed name's value)
void put_rep(std::vector<uint8_t>& o, const Rep& r) {
    if (r.form == kLiteral)
        o.push_back(0x40);
    else if (r.form == kIndexedName)
        put_integer(o, r.index, 4, 0x00);
    else
        put_integer(o, r.index, 7, 0x80);
}

// encode_string_literal (encoder.rs:299-307); with huffman, the H-bit form when strictly shorter
void put_string(std::vector<uint8_t>& o, const uint8_t* s, size_t n, int huffman) {
    if (huffman && n) {
        const size_t hl = hpk_huffman_encoded_len(s, n);
        if (hl < n) {
            put_integer(o, hl, 7, 0x80);
            const size_t at = o.size();
            o.resize(at + hl);
            size_t got = 0;
            hpk_huffman_encode_one(s, n, o.data() + at, hl, &got);
            return;
        }
    }
    put_integer(o, n, 7, 0);
    o.insert(o.end(), s, s + n);
}

}  // namespace

extern "C" hpk_henc* hpk_henc_create(int huffman) {
    hpk_henc* e = new (std::nothrow) hpk_henc();
    if (e) e->huffman = huffman ? 1 : 0;
    return e;
}

extern "C" void hpk_henc_destroy(hpk_henc* e) { delete e; }

extern "C" int hpk_henc_set_max_table_size(hpk_henc* e, size_t n) {
    if (!e) return HPK_E_INVAL;
    e->max_size = n;
    e->consolidate();
    return HPK_E_OK;
}

extern "C" int hpk_henc_table_size(const hpk_henc* e, size_t* size, size_t* entries, size_t* max_size) {
    if (!e) return HPK_E_INVAL;
    if (size) *size = e->size;
    if (entries) *entries = e->table.size();
    if (max_size) *max_size = e->max_size;
    return HPK_E_OK;
}

extern "C" int hpk_henc_encode(hpk_henc* e, const uint8_t* fields, const uint32_t* field_off, size_t n, uint8_t* out,
                               size_t cap, size_t* out_len) {
    if (!e || !out_len || (n && !field_off) || (cap && !out)) return HPK_E_INVAL;
    for (size_t k = 0; k < 2 * n; ++k)
        if (field_off[k + 1] < field_off[k]) return HPK_E_INVAL;
    if (n && field_off[2 * n] > field_off[0] && !fields) return HPK_E_INVAL;
    // encode against a copy of the state; commit only when the block fits
    hpk_henc next = *e;
    std::vector<uint8_t> o;
    for (size_t j = 0; j < n; ++j) {
        const uint8_t* nm = fields + field_off[2 * j];
        const size_t nl = field_off[2 * j + 1] - field_off[2 * j];
        const uint8_t* v = fields + field_off[2 * j + 1];
        const size_t vl = field_off[2 * j + 2] - field_off[2 * j + 1];
        const Rep r = next.choose(nm, nl, v, vl);
        put_rep(o, r);
        if (r.form == kLiteral) put_string(o, nm, nl, next.huffman);
        if (r.form != kIndexed) put_string(o, v, vl, next.huffman);
    }
    *out_len = o.size();
    if (o.size() > cap) return HPK_E_NOSPACE;
    if (!o.empty()) memcpy(out, o.data(), o.size());
    *e = std::move(next);
    return HPK_E_OK;
}

// Test hook (include/hpk.h): the next n Huffman batches made by hpk_henc_encode_blocks fail as a
// device error would, so tests can check that a failed call leaves every encoder as it was.
static thread_local int t_fail_batches = 0;
extern "C" void hpk_test_fail_batches(int n) { t_fail_batches = n > 0 ? n : 0; }

int hpk_test_take_failure() {  // -> 0, or the error of a batch the hook makes fail (hpk_internal.h)
    if (t_fail_batches <= 0) return 0;
    --t_fail_batches;
    return hpk_set_err_msg("injected batch failure (hpk_test_fail_batches)", HPK_E_DEVICE);
}

namespace {

int injected_failure() { return hpk_test_take_failure(); }

// What the device-plan path sends up: the arena (the static text, every encoder's live entries' bytes, the fields), and over it the
// tables, the fields' offsets from the first field's and the blocks' header offsets from the first block's.
struct PlanIn {
    std::vector<hpk_dtab> tabs;
    std::vector<uint8_t> flags, arena;
    std::vector<hpk_header> ent;
    std::vector<uint32_t> lfo, lhdr;
    uint64_t fields_base = 0, prefix_base = 0, nent = 0;  // (nent: the tables' records, ent's size unless 0)
};

// -> false: deferral is the host's to see (a table beyond the device ring, or offsets beyond the u32 range)
bool plan_inputs(const hpk_groups<hpk_henc>& g, const uint8_t* fields, const uint32_t* field_off, const uint32_t* hdr_off, uint32_t nblocks,
                 PlanIn* x) {
    const uint32_t ne = (uint32_t)g.who.size(), h0 = hdr_off[0], nh = hdr_off[nblocks] - h0;
    uint32_t ring = 0, chunk = 0, wge = 0, grp = 0;
    (void)hpk_test_blkplan_geometry(&ring, &chunk, &wge, &grp);
    const uint8_t* stext = nullptr;
    size_t slen = 0;
    (void)hpk_static_table(&stext, &slen, nullptr);
    // the tables: an encoder gets the records its max_size can ever fill
    x->tabs.resize(ne);
    x->flags.resize(ne);
    uint64_t& nent = x->nent;
    uint64_t prior = 0;
    for (uint32_t e = 0; e < ne; ++e) {
        const hpk_henc& h = *g.who[e];
        if (h.max_size > 32ull * ring || h.table.size() > ring) return false;
        const uint32_t need = (uint32_t)((h.max_size + 31) / 32), cnt = (uint32_t)h.table.size();
        const uint32_t cap = std::min(ring, std::max(need, cnt));
        x->tabs[e] = hpk_dtab{(uint32_t)nent, cap, cnt, (uint32_t)h.size, (uint32_t)h.max_size, HPK_DTAB_NO_LIMIT, 0u, 0u};
        x->flags[e] = (uint8_t)(h.huffman ? 1 : 0);
        nent += cap;
        prior += h.size - 32ull * cnt;
    }
    const uint32_t f_lo = field_off[2 * (size_t)h0];
    const uint64_t fbytes = field_off[2 * (size_t)hdr_off[nblocks]] - f_lo;
    x->fields_base = slen + prior;
    x->prefix_base = (x->fields_base + fbytes + 3) & ~3ull;
    if (x->prefix_base + 4ull * nh > HPK_MAX_OFFSET || fbytes + 4ull * nh + 18ull * nh > HPK_MAX_OFFSET || nent > 0x7FFFFFFFu ||
        nh >= 0x20000000u)
        return false;
    x->arena.resize(x->prefix_base);
    x->ent.resize(nent ? nent : 1);
    memcpy(x->arena.data(), stext, slen);
    size_t at = slen;
    for (uint32_t e = 0; e < ne; ++e) {
        hpk_header* rec = x->ent.data() + x->tabs[e].ent;
        for (const auto& kv : g.who[e]->table) {
            *rec++ = hpk_header{(uint32_t)at, (uint32_t)kv.first.size(), (uint32_t)(at + kv.first.size()), (uint32_t)kv.second.size()};
            memcpy(x->arena.data() + at, kv.first.data(), kv.first.size());
            memcpy(x->arena.data() + at + kv.first.size(), kv.second.data(), kv.second.size());
            at += kv.first.size() + kv.second.size();
        }
    }
    if (fbytes) memcpy(x->arena.data() + x->fields_base, fields + f_lo, fbytes);
    x->lfo.resize(2 * (size_t)nh + 1);
    for (size_t k = 0; k <= 2 * (size_t)nh; ++k) x->lfo[k] = field_off[2 * (size_t)h0 + k] - f_lo;
    x->lhdr.resize(nblocks + 1);
    for (uint32_t b = 0; b <= nblocks; ++b) x->lhdr[b] = hdr_off[b] - h0;
    return true;
}

// hpk_henc_encode_blocks with HPK_BLOCK_PLAN_DEVICE (include/hpk.h has the steps); the arguments are checked. Returns
// HPK_E_OK with `out` filled and every encoder's table rebuilt, a negative error with every encoder as it was, or 1:
// the host path is to answer the call (nothing has been touched).
int encode_blocks_planned(hpk_ctx* ctx, const hpk_groups<hpk_henc>& g, const uint8_t* fields, const uint32_t* field_off,
                          const uint32_t* hdr_off, uint32_t nblocks, hpk_henc_out* out) {
    const uint32_t ne = (uint32_t)g.who.size(), nh = hdr_off[nblocks] - hdr_off[0];
    if (!nh) return 1;
    PlanIn x;
    if (!plan_inputs(g, fields, field_off, hdr_off, nblocks, &x)) return 1;
    if (int rc = injected_failure()) return rc;
    out->block_off = (uint32_t*)malloc((nblocks + 1) * sizeof(uint32_t));
    if (!out->block_off) return HPK_E_INVAL;
    hpk_planjob job{};
    job.arena = x.arena.data();
    job.fields_base = (uint32_t)x.fields_base;
    job.prefix_base = (uint32_t)x.prefix_base;
    job.field_off = x.lfo.data();
    job.hdr_off = x.lhdr.data();
    job.nblocks = nblocks;
    job.nh = nh;
    job.enc_blk_off = g.off.data();
    job.enc_blk = g.list.data();
    job.enc_flags = x.flags.data();
    job.nencs = ne;
    job.tabs = x.tabs.data();
    job.tab_ent = x.ent.data();
    job.nent = (uint32_t)x.nent;
    job.block_off = out->block_off;
    int rc = hpk_plan_device(ctx, &job);
    if (getenv("HPK_HENC_TIMING"))
        fprintf(stderr, "hpk_henc plan path: up %ld us, plan %ld us, items %ld us, strings %ld us, back %ld us\n", job.us_up, job.us_plan,
                job.us_items, job.us_strings, job.us_back);
    auto give_up = [&](int code) {
        free(job.bytes);
        hpk_henc_out_free(out);
        return code;
    };
    bool whole = true;
    for (uint32_t e = 0; e < ne && !rc; ++e) whole &= x.tabs[e].applied == g.off[e + 1] - g.off[e];
    if (rc || !whole) return give_up(rc ? rc : 1);
    // every table rebuilt from its final entries' bytes, all of which lie in the host's arena; then the commit
    std::vector<std::deque<std::pair<std::string, std::string>>> fresh(ne);
    for (uint32_t e = 0; e < ne; ++e) {
        const hpk_header* rec = x.ent.data() + x.tabs[e].ent;
        for (uint32_t i = 0; i < x.tabs[e].count; ++i) {
            const hpk_header& r = rec[i];
            if ((uint64_t)r.name_off + r.name_len > x.arena.size() || (uint64_t)r.value_off + r.value_len > x.arena.size())
                return give_up(hpk_set_err_msg("the block plan returned an entry outside the arena", HPK_E_DEVICE));
            fresh[e].emplace_back(std::string((const char*)x.arena.data() + r.name_off, r.name_len),
                                  std::string((const char*)x.arena.data() + r.value_off, r.value_len));
        }
    }
    for (uint32_t e = 0; e < ne; ++e) {
        g.who[e]->table = std::move(fresh[e]);
        g.who[e]->size = x.tabs[e].size;
    }
    hpk_ctx_plan_answered(ctx);
    out->bytes = job.bytes;
    out->len = out->block_off[nblocks];
    out->n_blocks = nblocks;
    return HPK_E_OK;
}

// Pass 1's result: every block as a run of ops, each either octets that are final already (the representations'
// own, in `raw`) or a string literal still to be coded (the string list; string k = fields[s_at[k] .. + s_len[k])).
struct Op {
    uint32_t raw_at, raw_len;
    uint32_t str;  // index into the string list, or UINT32_MAX
};
struct Ops {
    std::vector<uint8_t> raw;
    std::vector<Op> ops;
    std::vector<uint32_t> ops_off;  // block b: ops[ops_off[b] .. ops_off[b + 1])
    std::vector<uint32_t> s_at, s_len;
    std::vector<uint8_t> s_huff;  // its encoder Huffman-codes
};

// pass 1: the representation of every header, against the working copies (block b's is work[of[b]])
Ops plan_ops(std::vector<hpk_henc>& work, const std::vector<uint32_t>& of, const uint8_t* fields, const uint32_t* field_off,
             const uint32_t* hdr_off, uint32_t nblocks) {
    Ops p;
    p.ops_off.assign(nblocks + 1, 0);
    for (uint32_t b = 0; b < nblocks; ++b) {
        hpk_henc& e = work[of[b]];
        auto lit = [&](uint32_t at, uint32_t len) {
            p.ops.push_back(Op{(uint32_t)p.raw.size(), 0u, (uint32_t)p.s_at.size()});
            p.s_at.push_back(at);
            p.s_len.push_back(len);
            p.s_huff.push_back((uint8_t)(e.huffman && len));
        };
        for (uint32_t j = hdr_off[b]; j < hdr_off[b + 1]; ++j) {
            const uint32_t na = field_off[2 * j], nl = field_off[2 * j + 1] - na;
            const uint32_t va = field_off[2 * j + 1], vl = field_off[2 * j + 2] - va;
            const Rep r = e.choose(fields + na, nl, fields + va, vl);
            const uint32_t r0 = (uint32_t)p.raw.size();
            put_rep(p.raw, r);
            p.ops.push_back(Op{r0, (uint32_t)p.raw.size() - r0, UINT32_MAX});
            if (r.form == kLiteral) lit(na, nl);
            if (r.form != kIndexed) lit(va, vl);
        }
        p.ops_off[b + 1] = (uint32_t)p.ops.size();
    }
    return p;
}

bool alloc_out(hpk_henc_out* out, uint32_t nblocks, size_t cap) {  // the caller's buffers (hpk_henc_out_free)
    out->block_off = (uint32_t*)malloc((nblocks + 1) * sizeof(uint32_t));
    out->bytes = (uint8_t*)malloc(cap ? cap : 1);
    if (out->block_off && out->bytes) return true;
    hpk_henc_out_free(out);
    return false;
}

// pass 2 on the device: every op in order is one item of ONE hpk_encode_strings_packed call, final
// representation octets as HPK_STR_VERBATIM, a string as HPK_STR_AUTO if its encoder Huffman-codes,
// else HPK_STR_RAW. The call's output is the blocks end to end: there is no pass 3.
int code_ops_device(hpk_ctx* ctx, const Ops& p, const uint8_t* fields, uint32_t nblocks, hpk_henc_out* out) {
    const size_t ni = p.ops.size();
    std::vector<uint32_t> in_off(ni + 1, 0), o_off(ni + 1), o_len(ni);
    std::vector<uint8_t> in, pol(ni), ist(ni);
    uint64_t hs = 0, eo_sum = 0;  // (the u32-range rule of the host path, on the same strings)
    for (size_t q = 0; q < ni; ++q) {
        const Op& op = p.ops[q];
        if (op.str == UINT32_MAX) {
            in.insert(in.end(), p.raw.begin() + op.raw_at, p.raw.begin() + op.raw_at + op.raw_len);
            pol[q] = HPK_STR_VERBATIM;
        } else {
            const uint32_t k = op.str;
            in.insert(in.end(), fields + p.s_at[k], fields + p.s_at[k] + p.s_len[k]);
            pol[q] = p.s_huff[k] ? HPK_STR_AUTO : HPK_STR_RAW;
            if (p.s_huff[k]) {
                hs += p.s_len[k];
                eo_sum += (hpk_encoded_bound(p.s_len[k]) + 3) & ~(uint64_t)3;
            }
        }
        if (hs > HPK_MAX_OFFSET || eo_sum > HPK_MAX_OFFSET || in.size() + 6 * (q + 1) > HPK_MAX_OFFSET)
            return hpk_set_err_msg("Huffman strings of one call exceed the u32 offset range", HPK_E_INVAL);
        in_off[q + 1] = (uint32_t)in.size();
    }
    if (int rc = injected_failure()) return rc;
    const size_t cap = in.size() + 6 * ni;
    if (!alloc_out(out, nblocks, cap)) return HPK_E_INVAL;
    if (int rc = hpk_encode_strings_packed(ctx, in.data(), in.size(), in_off.data(), (uint32_t)ni, pol.data(), out->bytes, cap,
                                           o_off.data(), o_len.data(), ist.data(), HPK_PTR_HOST)) {
        hpk_henc_out_free(out);
        return rc;
    }
    for (uint32_t b = 0; b <= nblocks; ++b) out->block_off[b] = o_off[p.ops_off[b]];
    out->n_blocks = nblocks;
    out->len = o_off[ni];
    return HPK_E_OK;
}

// pass 2 on the host (no context, or no string to Huffman-code): one Huffman batch on the library's CPU batch path
// for the strings of Huffman-coding encoders (u32 offsets: the strings and their encoded bounds must each fit below
// HPK_MAX_OFFSET); then pass 3: every block assembled.
int code_ops_host(const Ops& p, const uint8_t* fields, uint32_t nblocks, hpk_henc_out* out) {
    const uint32_t ns = (uint32_t)p.s_at.size();
    std::vector<uint32_t> bi(ns, UINT32_MAX);  // string -> batch index
    std::vector<uint32_t> in_off(1, 0), eo(1, 0);
    std::vector<uint8_t> in;
    uint64_t eo_sum = 0;
    for (uint32_t k = 0; k < ns; ++k) {
        if (!p.s_huff[k]) continue;
        bi[k] = (uint32_t)in_off.size() - 1;
        in.insert(in.end(), fields + p.s_at[k], fields + p.s_at[k] + p.s_len[k]);
        eo_sum += (hpk_encoded_bound(p.s_len[k]) + 3) & ~(uint64_t)3;
        if (in.size() > HPK_MAX_OFFSET || eo_sum > HPK_MAX_OFFSET)
            return hpk_set_err_msg("Huffman strings of one call exceed the u32 offset range", HPK_E_INVAL);
        in_off.push_back((uint32_t)in.size());
        eo.push_back((uint32_t)eo_sum);
    }
    const uint32_t nb = (uint32_t)in_off.size() - 1;
    std::vector<uint8_t> enc(eo.back() ? eo.back() : 1), est(nb ? nb : 1);
    std::vector<uint32_t> elen(nb ? nb : 1);
    if (nb) {
        if (in.empty()) in.push_back(0);
        int rc = injected_failure();
        if (!rc) rc = hpk_encode_batch_cpu(in.data(), in_off.data(), nb, enc.data(), eo.data(), elen.data(), est.data(), 0);
        if (rc) return rc;
    }
    std::vector<uint8_t> o;
    o.reserve(p.raw.size() + in.size() + 16);
    std::vector<uint32_t> boff(nblocks + 1, 0);
    for (uint32_t b = 0; b < nblocks; ++b) {
        for (uint32_t q = p.ops_off[b]; q < p.ops_off[b + 1]; ++q) {
            const Op& op = p.ops[q];
            if (op.str == UINT32_MAX) {
                o.insert(o.end(), p.raw.begin() + op.raw_at, p.raw.begin() + op.raw_at + op.raw_len);
                continue;
            }
            const uint32_t k = op.str, n = p.s_len[k];
            const uint32_t i = bi[k];
            if (i != UINT32_MAX && est[i] == HPK_OK && elen[i] < n) {  // the H-bit form, strictly shorter
                put_integer(o, elen[i], 7, 0x80);
                o.insert(o.end(), enc.begin() + eo[i], enc.begin() + eo[i] + elen[i]);
            } else {
                put_integer(o, n, 7, 0);
                o.insert(o.end(), fields + p.s_at[k], fields + p.s_at[k] + n);
            }
        }
        if (o.size() >= (1ull << 32)) return hpk_set_err_msg("encoded blocks exceed 4 GiB", HPK_E_INVAL);
        boff[b + 1] = (uint32_t)o.size();
    }
    if (!alloc_out(out, nblocks, o.size())) return HPK_E_INVAL;
    memcpy(out->block_off, boff.data(), (nblocks + 1) * sizeof(uint32_t));
    if (!o.empty()) memcpy(out->bytes, o.data(), o.size());
    out->n_blocks = nblocks;
    out->len = o.size();
    return HPK_E_OK;
}

}  // namespace

// Many response header blocks at once (the batched form of encoder.rs:210-234): the
// table logic runs per block on the host, in order per encoder (it never depends on how a string
// is coded); then, through ctx, every representation of every block is one item of ONE
// hpk_encode_strings_packed call whose output is the blocks end to end; without a ctx every string
// literal of every block whose encoder Huffman-codes is encoded in ONE batch on the library's CPU batch
// path and each block is assembled on the host. Either way the H-bit form is used wherever it is strictly
// shorter — the same bytes as hpk_henc_encode block by block: both take a header's representation from
// hpk_henc::choose.
extern "C" int hpk_henc_encode_blocks(hpk_ctx* ctx, hpk_henc* const* encs, const uint8_t* fields,
                                      const uint32_t* field_off, const uint32_t* hdr_off, uint32_t nblocks,
                                      hpk_henc_out* out) {
    if (!encs || !hdr_off || !out) return HPK_E_INVAL;
    memset(out, 0, sizeof *out);
    const uint32_t nh = hdr_off[nblocks] - hdr_off[0];
    for (uint32_t b = 0; b < nblocks; ++b)
        if (!encs[b] || hdr_off[b + 1] < hdr_off[b]) return HPK_E_INVAL;
    if (nh && !field_off) return HPK_E_INVAL;
    for (uint32_t k = 2 * hdr_off[0]; k < 2 * hdr_off[nblocks]; ++k)
        if (field_off[k + 1] < field_off[k]) return HPK_E_INVAL;
    if (nh && field_off[2 * hdr_off[nblocks]] > field_off[2 * hdr_off[0]] && !fields) return HPK_E_INVAL;
    const hpk_groups<hpk_henc> g = hpk_group_blocks(encs, nblocks);
    if (ctx && hpk_ctx_block_plan(ctx) == HPK_BLOCK_PLAN_DEVICE) {  // opt-in: the table logic on the device too
        const int rc = encode_blocks_planned(ctx, g, fields, field_off, hdr_off, nblocks, out);
        if (rc <= 0) return rc;
    }
    // Pass 1 runs against a working copy of each distinct encoder (hpk_henc_encode's `next = *e`);
    // the copies replace the encoders only once every block is assembled, so a call that fails in
    // the Huffman batch or the assembly leaves each dynamic table as it was and the peer's decoder
    // never sees an index to an entry whose header was not sent.
    std::vector<hpk_henc> work;
    work.reserve(g.who.size());
    for (const hpk_henc* e : g.who) work.push_back(*e);
    const Ops p = plan_ops(work, g.of, fields, field_off, hdr_off, nblocks);
    bool any_huff = false;
    for (uint8_t x : p.s_huff) any_huff |= x != 0;
    const int rc = ctx && any_huff ? code_ops_device(ctx, p, fields, nblocks, out) : code_ops_host(p, fields, nblocks, out);
    if (rc) return rc;
    // commit: every encoder takes its working copy's table
    for (size_t k = 0; k < g.who.size(); ++k) *g.who[k] = std::move(work[k]);
    return HPK_E_OK;
}

extern "C" void hpk_henc_out_free(hpk_henc_out* out) {
    if (!out) return;
    free(out->bytes);
    free(out->block_off);
    memset(out, 0, sizeof *out);
}
