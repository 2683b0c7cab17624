// hpk_h2.cpp — HTTP/2 frame layer in front of the two-pass HPACK decoder. Host code:
// the C ABI's hpk_h2_* entry points (include/hpk.h).
//
// The reference reads header blocks one connection and one stream at a time: its deframer
// (crates/loona/src/h2/server.rs:290-390) cuts frames (Frame::parse, crates/loona-h2/src/lib.rs:
// 397-411), drops the padding of DATA / HEADERS frames, the frame loop strips a HEADERS frame's
// priority block (server.rs:895-911), and read_headers (server.rs:1349-1643) gathers CONTINUATION
// fragments until END_HEADERS (lib.rs:139-168) and calls Decoder::decode_with_cb on the
// concatenation (server.rs:1619-1638). Here one call takes the bytes received on MANY connections,
// does the same framing per connection, and decodes every complete header block of every
// connection with ONE hpk_hdec_decode_blocks call: all their Huffman strings go to the device as one
// batch. A block whose CONTINUATION frames have not all arrived stays with its connection until a
// later call completes it; a connection error stops that connection, as the reference's connection
// task ends with GOAWAY.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <new>
#include <vector>

#include "../../include/hpk.h"
#include "hpk_internal.h"

int hpk_set_err_msg(const char* what, int code);  // hpk_ctx.hip: hpk_last_error's message

namespace {

enum : uint8_t { kData = 0x0, kHeaders = 0x1, kContinuation = 0x9 };
enum : uint8_t { kEndStream = 0x01, kEndHeaders = 0x04, kPadded = 0x08, kPriority = 0x20 };

uint32_t be24(const uint8_t* p) { return ((uint32_t)p[0] << 16) | ((uint32_t)p[1] << 8) | p[2]; }
uint32_t be31(const uint8_t* p) {
    return (((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]) & 0x7FFFFFFFu;
}

}  // namespace

struct hpk_h2conn {
    hpk_hdec* dec = nullptr;
    uint32_t max_frame_size = 16384;  // RFC 9113 §6.5.2 SETTINGS_MAX_FRAME_SIZE initial value
    // a HEADERS block still waiting for CONTINUATION frames (possibly across calls)
    bool pending = false;
    uint32_t pend_stream = 0;
    uint32_t pend_end_stream = 0;
    std::vector<uint8_t> frag;
    int32_t error = HPK_H2_OK;  // sticky: the reference's connection is gone after its first error
};

extern "C" hpk_h2conn* hpk_h2conn_create(void) {
    hpk_h2conn* c = new (std::nothrow) hpk_h2conn();
    if (!c) return nullptr;
    c->dec = hpk_hdec_create();
    if (!c->dec) {
        delete c;
        return nullptr;
    }
    return c;
}

extern "C" void hpk_h2conn_destroy(hpk_h2conn* c) {
    if (!c) return;
    hpk_hdec_destroy(c->dec);
    delete c;
}

extern "C" hpk_hdec* hpk_h2conn_decoder(hpk_h2conn* c) { return c ? c->dec : nullptr; }

extern "C" int hpk_h2conn_set_max_frame_size(hpk_h2conn* c, uint32_t n) {
    if (!c || n < 16384 || n > 16777215) return HPK_E_INVAL;  // RFC 9113 §6.5.2 bounds
    c->max_frame_size = n;
    return HPK_E_OK;
}

extern "C" int hpk_h2conn_error(const hpk_h2conn* c) { return c ? c->error : HPK_E_INVAL; }

extern "C" int hpk_h2_error_code(int err) {  // H2ConnectionError::as_known_error_code (types.rs:428-456)
    switch (err) {
        case HPK_H2_OK: return 0x0;                             // NO_ERROR
        case HPK_H2_FRAME_TOO_LARGE:                            // FRAME_SIZE_ERROR
        case HPK_H2_PADDED_FRAME_EMPTY: return 0x6;
        case HPK_H2_COMPRESSION_ERROR: return 0x9;              // COMPRESSION_ERROR
        default: return 0x1;                                    // PROTOCOL_ERROR
    }
}

// The device half's frame scan (hpk_internal.h: hpk_frames_device), installed by hpk_ctx_create; null where only
// the host half is linked. The host units name no symbol of the device half for it.
static std::atomic<hpk_frames_device_fn> g_frames_device{nullptr};
void hpk_h2_set_frames_device(hpk_frames_device_fn fn) { g_frames_device.store(fn, std::memory_order_relaxed); }

// Step 1 of hpk_h2_read_frames through the device (HPK_FRAME_SCAN_DEVICE): the states and the held fragment bytes
// of the pending connections are laid out as hpk_scan_frames takes them, the device function answers, and only then
// are the connections written: their states from the scan's, their held bytes from the open windows (a window at
// or past off[nconn] lies in the bytes held before). -> HPK_E_OK, HPK_FRAMES_NOT_SELECTED with nothing done (the
// function, asked with no job, says whether the context selects it), or a
// negative code with no connection touched. A connection listed twice in one call is HPK_E_INVAL on this path: the
// lanes walk the connections independently.
static int frames_on_device(hpk_frames_device_fn fn, hpk_ctx* ctx, hpk_h2conn* const* conns, const uint8_t* bytes,
                            const uint32_t* off, uint32_t nconn, hpk_h2_out* out, std::vector<uint8_t>& blk,
                            std::vector<uint32_t>& boff, std::vector<hpk_hdec*>& decs, std::vector<hpk_h2_block>& meta,
                            std::vector<int32_t>& frame_err) {
    if (fn(ctx, nullptr) != HPK_E_OK) return HPK_FRAMES_NOT_SELECTED;
    {
        std::vector<const hpk_h2conn*> seen(conns, conns + nconn);
        std::sort(seen.begin(), seen.end());
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return HPK_E_INVAL;
    }
    const uint32_t hi = off[nconn];
    std::vector<hpk_fconn> st(nconn);
    std::vector<uint8_t> carry;
    std::vector<uint32_t> coo((size_t)nconn + 1, 0);
    for (uint32_t c = 0; c < nconn; ++c) {
        const hpk_h2conn* k = conns[c];
        st[c] = hpk_fconn{k->max_frame_size, k->error, k->pending ? 1u : 0u, k->pend_stream | (k->pend_end_stream << 31), 0u, 0u, 0u, 0u};
        if (!k->pending) continue;
        if ((uint64_t)hi + carry.size() + k->frag.size() > HPK_MAX_OFFSET) return HPK_E_INVAL;
        st[c].carry_off = hi + (uint32_t)carry.size();
        st[c].carry_len = (uint32_t)k->frag.size();
        carry.insert(carry.end(), k->frag.begin(), k->frag.end());
    }
    hpk_frmjob job{};
    job.bytes = bytes;
    job.off = off;
    job.nconn = nconn;
    job.conns = st.data();
    job.carry = carry.data();
    job.ncarry = (uint32_t)carry.size();
    job.conn_open_off = coo.data();
    if (const int rc = fn(ctx, &job)) return rc;  // (failed: nothing was written)
    // everything is back: the new held bytes first (they read the old ones), then the connections
    std::vector<std::vector<uint8_t>> held(nconn);
    for (uint32_t c = 0; c < nconn; ++c)
        for (uint32_t w = coo[c]; w < coo[c + 1]; ++w) {
            const uint32_t a = job.open_off[w], n = job.open_len[w];
            const uint8_t* p = a >= hi ? carry.data() + (a - hi) : bytes + a;
            held[c].insert(held[c].end(), p, p + n);
        }
    for (uint32_t c = 0; c < nconn; ++c) {
        hpk_h2conn* k = conns[c];
        k->error = st[c].error;
        k->pending = st[c].pending != 0;
        k->pend_stream = st[c].pend_stream & 0x7FFFFFFFu;
        k->pend_end_stream = st[c].pend_stream >> 31;
        k->frag.swap(held[c]);
        out->conn_consumed[c] = st[c].consumed;
        frame_err[c] = st[c].error;
    }
    const uint32_t nb = job.nblocks;
    blk.assign(job.blk, job.blk + job.block_off[nb]);
    boff.assign(job.block_off, job.block_off + nb + 1);
    for (uint32_t b = 0; b < nb; ++b) {
        const hpk_fblock& f = job.blocks[b];
        decs.push_back(conns[f.conn]->dec);
        meta.push_back(hpk_h2_block{f.conn, f.stream_id & 0x7FFFFFFFu, f.stream_id >> 31, 0u});
    }
    free(job.blocks), free(job.block_off), free(job.blk), free(job.open_off), free(job.open_len);
    return HPK_E_OK;
}

extern "C" int hpk_h2_read_frames(hpk_ctx* ctx, hpk_h2conn* const* conns, const uint8_t* bytes, const uint32_t* off,
                                  uint32_t nconn, hpk_h2_out* out) {
    if (!conns || !off || !out || (nconn && off[nconn] > off[0] && !bytes)) return HPK_E_INVAL;
    memset(out, 0, sizeof *out);
    for (uint32_t c = 0; c < nconn; ++c)
        if (!conns[c] || off[c + 1] < off[c]) return HPK_E_INVAL;
    out->n_conns = nconn;
    out->conn_error = (int32_t*)calloc(nconn ? nconn : 1, sizeof(int32_t));
    out->conn_consumed = (uint32_t*)calloc(nconn ? nconn : 1, sizeof(uint32_t));
    if (!out->conn_error || !out->conn_consumed) {
        hpk_h2_out_free(out);
        return HPK_E_INVAL;
    }
    // 1. framing, connection by connection: complete header blocks are copied into one buffer
    std::vector<uint8_t> blk;
    std::vector<uint32_t> boff(1, 0);
    std::vector<hpk_hdec*> decs;
    std::vector<hpk_h2_block> meta;
    blk.reserve(off[nconn] - off[0]);
    auto emit = [&](uint32_t c, uint32_t sid, uint32_t end_stream, const uint8_t* p, size_t n) {
        blk.insert(blk.end(), p, p + n);
        boff.push_back((uint32_t)blk.size());
        decs.push_back(conns[c]->dec);
        meta.push_back(hpk_h2_block{c, sid, end_stream, 0u});
    };
    std::vector<int32_t> frame_err(nconn, HPK_H2_OK);  // framing errors found this call
    // with a context on HPK_FRAME_SCAN_DEVICE the device does this step (include/hpk.h); else the loop below
    int on_device = HPK_FRAMES_NOT_SELECTED;
    if (const hpk_frames_device_fn fn = ctx ? g_frames_device.load(std::memory_order_relaxed) : nullptr) {
        on_device = frames_on_device(fn, ctx, conns, bytes, off, nconn, out, blk, boff, decs, meta, frame_err);
        if (on_device < 0) {
            hpk_h2_out_free(out);
            return on_device;
        }
    }
    for (uint32_t c = 0; on_device == HPK_FRAMES_NOT_SELECTED && c < nconn; ++c) {
        hpk_h2conn* k = conns[c];
        size_t pos = off[c];
        const size_t end = off[c + 1];
        int32_t err = k->error;
        while (err == HPK_H2_OK && end - pos >= 9) {
            const uint8_t* h = bytes + pos;
            const uint32_t len = be24(h), sid = be31(h + 5);
            const uint8_t type = h[3], flags = h[4];
            if (len > k->max_frame_size) {  // server.rs:318-325
                err = HPK_H2_FRAME_TOO_LARGE;
                break;
            }
            if (end - pos - 9 < len) break;  // the rest of this frame comes with a later call
            const uint8_t* p = h + 9;
            size_t n = len;
            pos += 9 + (size_t)len;
            if ((type == kData || type == kHeaders) && (flags & kPadded)) {  // server.rs:356-382
                if (n == 0) {
                    err = HPK_H2_PADDED_FRAME_EMPTY;
                    break;
                }
                const size_t pad = p[0];
                p += 1;
                n -= 1;
                if (n < pad) {
                    err = HPK_H2_PADDED_FRAME_TOO_SHORT;
                    break;
                }
                n -= pad;
            }
            if (k->pending) {  // read_headers' CONTINUATION loop (server.rs:1376-1417)
                // the stream id is checked before the frame type (server.rs:1391-1397, then 1399-1408):
                // any frame of another stream is ExpectedContinuationForStream, whatever its type
                if (sid != k->pend_stream) {
                    err = HPK_H2_EXPECTED_CONTINUATION_FOR_STREAM;
                    break;
                }
                if (type != kContinuation) {
                    err = HPK_H2_EXPECTED_CONTINUATION_FRAME;
                    break;
                }
                k->frag.insert(k->frag.end(), p, p + n);
                if (flags & kEndHeaders) {
                    emit(c, k->pend_stream, k->pend_end_stream, k->frag.data(), k->frag.size());
                    k->pending = false;
                    k->frag.clear();
                }
                continue;
            }
            if (type == kContinuation) {  // server.rs:1299-1303
                err = HPK_H2_UNEXPECTED_CONTINUATION_FRAME;
                break;
            }
            if (type != kHeaders) continue;  // other frame types: not this layer's business
            if (flags & kPriority) {         // server.rs:895-911, PrioritySpec::parse
                if (n < 5) {
                    err = HPK_H2_PRIORITY_PARSE;
                    break;
                }
                if (be31(p) == sid) {
                    err = HPK_H2_HEADERS_INVALID_PRIORITY;
                    break;
                }
                p += 5;
                n -= 5;
            }
            const uint32_t es = (flags & kEndStream) ? 1u : 0u;
            if (flags & kEndHeaders) {
                emit(c, sid, es, p, n);
            } else {
                k->pending = true;
                k->pend_stream = sid;
                k->pend_end_stream = es;
                k->frag.assign(p, p + n);
            }
        }
        out->conn_consumed[c] = (uint32_t)(pos - off[c]);
        frame_err[c] = err;
        if (err != HPK_H2_OK) k->error = err;
    }
    // 2. every complete block of every connection in one two-pass decode (one Huffman batch)
    const uint32_t nb = (uint32_t)meta.size();
    int rc = nb ? hpk_hdec_decode_blocks(ctx, decs.data(), blk.data(), boff.data(), nb, &out->hb) : HPK_E_OK;
    if (rc) {
        hpk_h2_out_free(out);
        return rc;
    }
    out->blocks = (hpk_h2_block*)malloc((nb ? nb : 1) * sizeof(hpk_h2_block));
    if (!out->blocks) {
        hpk_h2_out_free(out);
        return HPK_E_INVAL;
    }
    if (nb) memcpy(out->blocks, meta.data(), nb * sizeof(hpk_h2_block));
    // 3. a decoding error is a connection error (COMPRESSION_ERROR, types.rs:446): it comes before
    // any framing error of the same call (its block was framed earlier), and the connection's
    // later blocks are never decoded by the reference
    std::vector<uint8_t> dead(nconn, 0);
    for (uint32_t c = 0; c < nconn; ++c) dead[c] = conns[c]->error != HPK_H2_OK && frame_err[c] == HPK_H2_OK;
    for (uint32_t b = 0; b < nb; ++b) {
        const uint32_t c = meta[b].conn;
        if (dead[c]) {
            out->blocks[b].skipped = 1;
            continue;
        }
        if (out->hb.blocks[b].error != HPK_BLK_OK) {
            dead[c] = 1;
            conns[c]->error = HPK_H2_COMPRESSION_ERROR;
            frame_err[c] = HPK_H2_COMPRESSION_ERROR;
        }
    }
    for (uint32_t c = 0; c < nconn; ++c) out->conn_error[c] = conns[c]->error;
    return HPK_E_OK;
}

extern "C" void hpk_h2_out_free(hpk_h2_out* out) {
    if (!out) return;
    hpk_blocks_out_free(&out->hb);
    free(out->blocks);
    free(out->conn_error);
    free(out->conn_consumed);
    memset(out, 0, sizeof *out);
}

// ---- the write side: header blocks to HEADERS and CONTINUATION frames --------------------------------------------
// The reference queues a response's header block in send_data_maybe (crates/loona/src/h2/server.rs:470-508): while
// the piece left is strictly longer than the peer's max frame size, a frame of that many octets without flags
// (HEADERS first, CONTINUATION after), then the last piece with END_HEADERS; Frame::write_into
// (crates/loona-h2/src/lib.rs:413-422) puts the 9-octet header in front of each.
namespace {

// one frame header to p
void put_frame_header(uint8_t* p, uint32_t len, uint8_t type, uint8_t flags, uint32_t sid) {
    p[0] = (uint8_t)(len >> 16), p[1] = (uint8_t)(len >> 8), p[2] = (uint8_t)len;
    p[3] = type, p[4] = flags;
    sid &= 0x7FFFFFFFu;
    p[5] = (uint8_t)(sid >> 24), p[6] = (uint8_t)(sid >> 16), p[7] = (uint8_t)(sid >> 8), p[8] = (uint8_t)sid;
}

// n octets from src to the wire position `at` of out, clipped at lim
void put_clipped(uint8_t* out, uint64_t at, uint64_t lim, const uint8_t* src, size_t n) {
    if (at >= lim || n == 0) return;
    memcpy(out + at, src, (size_t)(lim - at < n ? lim - at : n));
}

}  // namespace

extern "C" int hpk_write_frames_cpu(const uint8_t* blocks, size_t cap, const uint32_t* block_off, uint32_t nblocks,
                                    const uint32_t* stream_id, const uint32_t* max_frame, uint8_t* out_blob, size_t out_cap,
                                    uint32_t* wire_off, uint8_t* status) {
    if (!block_off || !wire_off || (nblocks && (!stream_id || !max_frame || !status))) return hpk_set_err_msg("null argument", HPK_E_INVAL);
    if (nblocks >= 0x7FFFFFFFu) return hpk_set_err_msg("too many blocks for the frame write", HPK_E_INVAL);
    if (cap > HPK_MAX_OFFSET) return hpk_set_err_msg("the frame write's blob passes HPK_MAX_OFFSET", HPK_E_INVAL);
    if (nblocks && ((!blocks && cap) || (!out_blob && out_cap))) return hpk_set_err_msg("null blob", HPK_E_INVAL);
    // the host-pointer rules: everything checked before anything is written
    for (uint32_t b = 0; b < nblocks; ++b)
        if (block_off[b + 1] < block_off[b]) return hpk_set_err_msg("offsets must be non-decreasing", HPK_E_INVAL);
    if (block_off[nblocks] > cap) return hpk_set_err_msg("offsets pass the blob's capacity", HPK_E_INVAL);
    uint64_t total = 0;
    for (uint32_t b = 0; b < nblocks; ++b) {
        if (!hpk_max_frame_ok(max_frame[b])) return hpk_set_err_msg("a max_frame of 0 or above 0xFFFFFF", HPK_E_INVAL);
        total += hpk_wire_len(block_off[b + 1] - block_off[b], max_frame[b]);
    }
    if (total > HPK_MAX_OFFSET) {  // every block void, as the device has it
        for (uint32_t b = 0; b <= nblocks; ++b) wire_off[b] = 0;
        for (uint32_t b = 0; b < nblocks; ++b) status[b] = HPK_BAD_OFFSETS;
        return hpk_set_err_msg("the wire octets pass HPK_MAX_OFFSET", HPK_E_INVAL);
    }
    const uint64_t lim = total < out_cap ? total : out_cap;
    uint64_t at = 0;
    for (uint32_t b = 0; b < nblocks; ++b) {
        wire_off[b] = (uint32_t)at;
        status[b] = HPK_OK;
        const uint8_t* p = blocks + block_off[b];
        size_t left = block_off[b + 1] - block_off[b];
        const uint32_t M = max_frame[b], sid = stream_id[b];
        bool first = true;
        for (;;) {  // server.rs:470-508
            const bool last = left <= M;
            const size_t n = last ? left : M;
            uint8_t h[9];
            put_frame_header(h, (uint32_t)n, first ? kHeaders : kContinuation, (uint8_t)((last ? kEndHeaders : 0) | (first && (sid >> 31) ? kEndStream : 0)), sid);
            put_clipped(out_blob, at, lim, h, 9);
            put_clipped(out_blob, at + 9, lim, p, n);
            at += 9 + n;
            p += n;
            left -= n;
            first = false;
            if (last) break;
        }
    }
    wire_off[nblocks] = (uint32_t)at;
    if (total > out_cap) return hpk_set_err_msg("the wire octets pass the output capacity", HPK_E_NOSPACE);
    return HPK_E_OK;
}

// The device half's frame write (hpk_internal.h: hpk_write_device), installed by hpk_ctx_create; null where only the
// host half is linked.
static std::atomic<hpk_write_device_fn> g_write_device{nullptr};
void hpk_h2_set_write_device(hpk_write_device_fn fn) { g_write_device.store(fn, std::memory_order_relaxed); }

extern "C" int hpk_h2_write_headers(hpk_ctx* ctx, hpk_henc* const* encs, const uint8_t* fields, const uint32_t* field_off,
                                    const uint32_t* hdr_off, uint32_t nblocks, const uint32_t* stream_id, const uint32_t* max_frame,
                                    hpk_henc_out* out) {
    if (!out) return HPK_E_INVAL;
    memset(out, 0, sizeof *out);
    if (nblocks && (!stream_id || !max_frame)) return hpk_set_err_msg("null argument", HPK_E_INVAL);
    for (uint32_t b = 0; b < nblocks; ++b)  // before anything else: the encoders stay as they are
        if (!hpk_max_frame_ok(max_frame[b])) return hpk_set_err_msg("a max_frame of 0 or above 0xFFFFFF", HPK_E_INVAL);
    hpk_henc_out blk;
    if (const int rc = hpk_henc_encode_blocks(ctx, encs, fields, field_off, hdr_off, nblocks, &blk)) return rc;
    // from here on the encoders' tables are committed
    static const uint32_t no_blocks[1] = {0};
    const uint32_t* boff = blk.block_off ? blk.block_off : no_blocks;
    uint64_t total = 0;
    for (uint32_t b = 0; b < nblocks; ++b) total += hpk_wire_len(boff[b + 1] - boff[b], max_frame[b]);
    int rc = HPK_E_OK;
    std::vector<uint8_t> status(nblocks ? nblocks : 1);
    if (total > HPK_MAX_OFFSET) rc = hpk_set_err_msg("the wire octets pass HPK_MAX_OFFSET", HPK_E_INVAL);
    if (!rc) {
        out->bytes = (uint8_t*)malloc(total ? (size_t)total : 1);
        out->block_off = (uint32_t*)malloc(((size_t)nblocks + 1) * sizeof(uint32_t));
        if (!out->bytes || !out->block_off) rc = hpk_set_err_msg("out of memory", HPK_E_INVAL);
    }
    if (!rc) {
        int on_device = HPK_FRAMES_NOT_SELECTED;
        if (const hpk_write_device_fn fn = ctx ? g_write_device.load(std::memory_order_relaxed) : nullptr)
            on_device = fn(ctx, blk.bytes, blk.len, boff, nblocks, stream_id, max_frame, out->bytes, (size_t)total, out->block_off,
                           status.data());
        if (on_device != HPK_E_OK)  // not selected, or it failed: the host framing answers
            rc = hpk_write_frames_cpu(blk.bytes, blk.len, boff, nblocks, stream_id, max_frame, out->bytes, (size_t)total,
                                      out->block_off, status.data());
    }
    hpk_henc_out_free(&blk);
    if (rc) {
        hpk_henc_out_free(out);
        return rc;
    }
    out->len = (size_t)total;
    out->n_blocks = nblocks;
    return HPK_E_OK;
}
