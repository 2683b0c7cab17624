// hpk_strparse.h — the per-thread code of the string-literal decode's parse step (hpk_decode_strings.hip):
// decode_string's front half (crates/loona-hpack/src/decoder.rs:135-143) on one window of the input blob: the
// 7-bit-prefix length integer (decode_integer, decoder.rs:67-125), the `consumed + len > buf.len()` check and
// the H bit. The payload is not touched. Nothing here touches memory except through the pointer it is given,
// so tests/emu/strparse_emu.cpp runs this function as it is on the host.
//
// Loads are byte loads, not pack_segment's aligned dwords with a range test: a string whose length is below
// 127 (nearly every header string) needs exactly its first octet, and an integer that crosses a dword
// boundary would need two dwords and the shift between them for the same one to five octets. Neighbouring
// threads' windows are a cache line apart or less, so the lines come in once either way. An octet is read only
// after it is known to lie inside the window, and the window inside the blob.
#pragma once
#include <stdint.h>

#include "../../include/hpk.h"

namespace hpkstr {

struct StrParse {
    uint32_t status;    // HPK_OK, HPK_BAD_OFFSETS, HPK_PREFIX_TOO_MANY_OCTETS, HPK_PREFIX_NOT_ENOUGH_OCTETS,
                        // HPK_STRING_NOT_ENOUGH_OCTETS
    uint32_t huff;      // the H bit (0 unless status is HPK_OK)
    uint32_t start;     // the payload's first byte, an offset into the blob
    uint32_t len;       // the payload's bytes
    uint32_t consumed;  // prefix octets + len; 0 unless status is HPK_OK
};

// The string whose window is blob[a .. e); cap: the blob's bytes. A window with a > e or e > cap is void
// (HPK_BAD_OFFSETS) and no byte is read.
template <class BP>
__device__ __forceinline__ StrParse str_parse(BP blob, uint32_t cap, uint32_t a, uint32_t e) {
    StrParse r = {HPK_BAD_OFFSETS, 0u, 0u, 0u, 0u};
    if (a > e || e > cap) return r;
    const uint32_t w = e - a;
    r.status = HPK_PREFIX_NOT_ENOUGH_OCTETS;
    if (w == 0u) return r;  // buf.is_empty()
    const uint32_t b0 = blob[a];
    uint32_t v = b0 & 127u, used = 1u;
    if (v == 127u) {  // the value does not fit the prefix: up to four more octets, 7 bits each, low bits first
        bool done = false;
#pragma unroll
        for (uint32_t k = 1; k < 5u; ++k) {
            if (done) break;
            if (k >= w) return r;  // the window ends inside the integer
            const uint32_t b = blob[a + k];
            used = k + 1u;
            v += (b & 127u) << (7u * (k - 1u));  // (at most 127 + 2^28 - 1)
            if (!(b & 128u)) {
                done = true;
            } else if (used == 5u) {  // the continuation bit still set on the 5th octet
                r.status = HPK_PREFIX_TOO_MANY_OCTETS;
                return r;
            }
        }
    }
    if ((uint64_t)used + v > (uint64_t)w) {  // consumed + len > buf.len()
        r.status = HPK_STRING_NOT_ENOUGH_OCTETS;
        return r;
    }
    r.status = HPK_OK;
    r.huff = b0 >> 7;
    r.start = a + used;
    r.len = v;
    r.consumed = used + v;
    return r;
}

}  // namespace hpkstr
