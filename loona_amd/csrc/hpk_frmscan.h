// hpk_frmscan.h — the per-lane code of the HTTP/2 frame scan (hpk_frmscan.hip, hpk_scan_frames): step 1 of
// hpk_h2_read_frames (hpk_h2.cpp) on one connection's bytes blob[lo .. hi): the deframer's length check and padding
// removal (crates/loona/src/h2/server.rs:290-390; Frame::parse, crates/loona-h2/src/lib.rs:397-411), the HEADERS
// priority block (server.rs:895-911), and read_headers' CONTINUATION gathering (server.rs:1299-1303, 1349-1417).
// Where a header block's fragments lie depends only on the connection's bytes and four words of state, so a
// connection is walked with no decoder in hand.
//
// One walk serves both passes and the CPU replay: it counts blocks and fragments itself and hands every fragment
// window and every completed block to a visitor. The count pass passes a visitor that does nothing, the emit pass
// one that stores; the two cannot disagree on what is where. Nothing here touches memory except through the pointer
// it is given, so tests/emu/frmscan_emu.cpp runs this code as it is on the host.
//
// Loads are byte loads, as hpk_blkscan.h's and for its reasons (a connection's lines come in once either way, and
// a frame header lies at any alignment). A payload is never read beyond its pad-length octet and its four
// dependency octets. An octet is read only after it is known to lie inside [lo, hi), and that inside the blob (the
// caller's check). The carry window is listed, never read.
#pragma once
#include <stdint.h>

#include "../../include/hpk.h"

namespace hpkfrm {

enum : uint32_t { kData = 0x0, kHeaders = 0x1, kContinuation = 0x9 };
enum : uint32_t { kEndStream = 0x01, kEndHeaders = 0x04, kPadded = 0x08, kPriority = 0x20 };

// the four words of a connection's state that the walk reads and updates (hpk_fconn's first four)
struct State {
    uint32_t max_frame_size;
    int32_t error;         // hpk_h2_error, sticky
    uint32_t pending;      // a HEADERS block waits for CONTINUATION
    uint32_t pend_stream;  // its stream id, bit 31 = the HEADERS frame's END_STREAM
};

struct Counts {
    uint32_t blocks;    // blocks completed in this walk
    uint32_t frags;     // every fragment handed over, the carry included
    uint32_t open;      // the trailing ones of those: the fragments of a block still pending at the end
    uint32_t consumed;  // bytes of whole frames consumed
};

// the count pass's visitor
struct NoVisit {
    __device__ __forceinline__ void fragment(uint32_t, uint32_t, uint32_t) {}
    __device__ __forceinline__ void block(uint32_t, uint32_t, uint32_t, uint32_t) {}
};

template <class BP>
__device__ __forceinline__ uint32_t be31(BP blob, uint32_t at) {
    return (((uint32_t)blob[at] << 24) | ((uint32_t)blob[at + 1u] << 16) | ((uint32_t)blob[at + 2u] << 8) | (uint32_t)blob[at + 3u]) &
           0x7FFFFFFFu;
}

// The connection's bytes blob[lo .. hi), lo <= hi <= HPK_MAX_OFFSET and hi within the blob (the caller's check); s
// comes in as the connection's state and leaves as its new state. vis.fragment(j, off, len): the connection's j-th
// fragment is blob[off .. off + len), exact (no padding, pad-length octet or priority block); a connection that
// enters pending has its carry window as fragment 0. vis.block(k, stream_id | END_STREAM << 31, first, nfrag): its
// k-th completed block is the fragments first .. first + nfrag, handed over before it. The fragments no block
// covers are the last Counts::open ones.
template <class BP, class V>
__device__ __forceinline__ Counts walk_frames(BP blob, uint32_t lo, uint32_t hi, State& s, uint32_t carry_off, uint32_t carry_len,
                                              V& vis) {
    Counts n = {0u, 0u, 0u, 0u};
    uint32_t first = 0u;  // the pending block's first fragment
    if (s.pending) {
        vis.fragment(0u, carry_off, carry_len);
        n.frags = 1u;
    }
    uint32_t pos = lo;
    int32_t err = s.error;
    while (err == HPK_H2_OK && hi - pos >= 9u) {
        const uint32_t len = ((uint32_t)blob[pos] << 16) | ((uint32_t)blob[pos + 1u] << 8) | (uint32_t)blob[pos + 2u];
        const uint32_t type = blob[pos + 3u], flags = blob[pos + 4u];
        const uint32_t sid = be31(blob, pos + 5u);
        if (len > s.max_frame_size) {  // server.rs:318-325; the frame is not consumed
            err = HPK_H2_FRAME_TOO_LARGE;
            break;
        }
        if (hi - pos - 9u < len) break;  // the rest of this frame comes with a later call
        uint32_t p = pos + 9u, m = len;
        pos += 9u + len;  // consumed, whatever this frame turns out to be
        if ((type == kData || type == kHeaders) && (flags & kPadded)) {  // server.rs:356-382
            if (m == 0u) {
                err = HPK_H2_PADDED_FRAME_EMPTY;
                break;
            }
            const uint32_t pad = blob[p];
            p += 1u;
            m -= 1u;
            if (m < pad) {
                err = HPK_H2_PADDED_FRAME_TOO_SHORT;
                break;
            }
            m -= pad;
        }
        if (s.pending) {  // read_headers' CONTINUATION loop (server.rs:1376-1417): the stream id first (1391-1397)
            if (sid != (s.pend_stream & 0x7FFFFFFFu)) {
                err = HPK_H2_EXPECTED_CONTINUATION_FOR_STREAM;
                break;
            }
            if (type != kContinuation) {  // server.rs:1399-1408
                err = HPK_H2_EXPECTED_CONTINUATION_FRAME;
                break;
            }
            vis.fragment(n.frags, p, m);
            n.frags += 1u;
            if (flags & kEndHeaders) {
                vis.block(n.blocks, s.pend_stream, first, n.frags - first);
                n.blocks += 1u;
                s.pending = 0u;
                first = n.frags;
            }
            continue;
        }
        if (type == kContinuation) {  // server.rs:1299-1303
            err = HPK_H2_UNEXPECTED_CONTINUATION_FRAME;
            break;
        }
        if (type != kHeaders) continue;  // other frame types: not this layer's business
        if (flags & kPriority) {         // server.rs:895-911, PrioritySpec::parse
            if (m < 5u) {
                err = HPK_H2_PRIORITY_PARSE;
                break;
            }
            if (be31(blob, p) == sid) {
                err = HPK_H2_HEADERS_INVALID_PRIORITY;
                break;
            }
            p += 5u;
            m -= 5u;
        }
        const uint32_t sid_es = sid | ((flags & kEndStream) ? 0x80000000u : 0u);
        vis.fragment(n.frags, p, m);
        n.frags += 1u;
        if (flags & kEndHeaders) {
            vis.block(n.blocks, sid_es, first, 1u);
            n.blocks += 1u;
            first = n.frags;
        } else {
            s.pending = 1u;
            s.pend_stream = sid_es;
        }
    }
    s.error = err;
    n.consumed = pos - lo;
    n.open = s.pending ? n.frags - first : 0u;
    return n;
}

// Whether connection [lo, hi) of a blob of cap bytes, with this carry window if it is pending, may be walked; a
// connection that may not is void (HPK_BAD_OFFSETS).
__device__ __forceinline__ bool conn_ok(uint32_t lo, uint32_t hi, uint32_t cap, uint32_t pending, uint32_t carry_off,
                                        uint32_t carry_len) {
    if (lo > hi || hi > cap) return false;
    return !pending || (carry_off <= cap && carry_len <= cap - carry_off);
}

}  // namespace hpkfrm
