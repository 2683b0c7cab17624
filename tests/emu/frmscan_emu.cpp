// host replay of the frame scan's two passes (loona_amd/csrc/hpk_frmscan.hip): the REAL per-lane walk of
// hpk_frmscan.h (walk_frames), one connection at a time, on connections read from a file that
// tests/test_frmscan_emulation.py writes (and whose answers it takes from frames_cases.ref_scan_frames).
//
// Every connection is walked in several placements, which must all agree:
//   * the count pass (the visitor that does nothing) and the emit pass (a visitor that collects) through a checking
//     accessor that counts any index outside the connection's range, the connection 5 bytes into a blob with poison
//     on both sides and its carry window behind that: the counts must be the collected sizes, and the state the two
//     passes leave the same;
//   * both passes through a plain pointer with the blob at the end of a buffer whose next page has no access, the
//     connection at each of the 4 dword alignments, once ending with the blob and once followed inside the blob by
//     poison bytes (0xFF: a frame header of the largest length, every flag set), the carry window in front of the
//     connection and poisoned too (it is listed, never read), so a read outside the connection changes the answer
//     or faults.
//   usage: frmscan_emu <cases file>
//   file: u32 count, then per case u32 max_frame_size, i32 error, u32 pending, u32 pend_stream, u32 carry length,
//   u32 data length, the data's bytes (the carry's bytes are not needed: the walk never reads them)
//   output: one line per case: nblocks nfrags nopen consumed error pending pend_stream, then per block sid_es first
//   nfrag, then per fragment off len (offsets relative to the connection's first byte; the carry window is printed
//   as the data's length)
#include "shim.h"
#include "hpk_frmscan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>

#include <vector>

using namespace hpkfrm;

static long g_bad = 0;

struct Checked {
    const uint8_t* p;
    uint32_t lo, hi;
    long* oob;
    uint8_t operator[](uint32_t i) const {
        if (i < lo || i >= hi) {
            ++*oob;
            return 0xFF;
        }
        return p[i];
    }
};

struct Blk {
    uint32_t sid_es, first, nfrag;
};
struct Frag {
    uint32_t off, len;
};

struct Collect {
    std::vector<Blk> blocks;
    std::vector<Frag> frags;
    long order_bad = 0;
    void fragment(uint32_t j, uint32_t off, uint32_t len) {
        if (j != frags.size()) ++order_bad;
        frags.push_back({off, len});
    }
    void block(uint32_t k, uint32_t sid_es, uint32_t first, uint32_t nfrag) {
        // a block's fragments are handed over before it, and the blocks tile what has been handed over
        const uint32_t done = blocks.empty() ? 0u : blocks.back().first + blocks.back().nfrag;
        if (k != blocks.size() || first != done || first + nfrag != frags.size() || nfrag == 0) ++order_bad;
        blocks.push_back({sid_es, first, nfrag});
    }
};

// what a walk gave, with every data offset counted from the connection's start `a` and the carry window named `len`
struct Answer {
    Counts n;
    State s;
    Collect c;
};

static bool same_state(const State& x, const State& y) {
    return x.max_frame_size == y.max_frame_size && x.error == y.error && x.pending == y.pending && x.pend_stream == y.pend_stream;
}

static bool same(const Answer& x, uint32_t ax, uint32_t cx, const Answer& y, uint32_t ay, uint32_t cy, uint32_t len, bool pending) {
    if (x.n.blocks != y.n.blocks || x.n.frags != y.n.frags || x.n.open != y.n.open || x.n.consumed != y.n.consumed) return false;
    if (!same_state(x.s, y.s) || x.c.blocks.size() != y.c.blocks.size() || x.c.frags.size() != y.c.frags.size()) return false;
    for (size_t i = 0; i < x.c.blocks.size(); ++i)
        if (x.c.blocks[i].sid_es != y.c.blocks[i].sid_es || x.c.blocks[i].first != y.c.blocks[i].first ||
            x.c.blocks[i].nfrag != y.c.blocks[i].nfrag)
            return false;
    for (size_t i = 0; i < x.c.frags.size(); ++i) {
        const bool carry = pending && i == 0;
        const uint32_t ox = carry ? x.c.frags[i].off - cx + len : x.c.frags[i].off - ax;
        const uint32_t oy = carry ? y.c.frags[i].off - cy + len : y.c.frags[i].off - ay;
        if (ox != oy || x.c.frags[i].len != y.c.frags[i].len) return false;
    }
    return true;
}

// both passes on blob[a .. a + len) with state st and the carry window (carry_off, carry_len); false if they disagree
template <class BP>
static bool both(BP blob, uint32_t a, uint32_t len, const State& st, uint32_t carry_off, uint32_t carry_len, Answer* out) {
    State s1 = st, s2 = st;
    NoVisit nv;
    const Counts c1 = walk_frames(blob, a, a + len, s1, carry_off, carry_len, nv);
    out->c = Collect();
    out->n = walk_frames(blob, a, a + len, s2, carry_off, carry_len, out->c);
    out->s = s2;
    const Counts& c2 = out->n;
    if (c1.blocks != c2.blocks || c1.frags != c2.frags || c1.open != c2.open || c1.consumed != c2.consumed || !same_state(s1, s2)) return false;
    if (c2.blocks != out->c.blocks.size() || c2.frags != out->c.frags.size() || out->c.order_bad) return false;
    // the open fragments are the ones behind the last block
    const uint32_t done = out->c.blocks.empty() ? 0u : out->c.blocks.back().first + out->c.blocks.back().nfrag;
    return c2.open == (s2.pending ? c2.frags - done : 0u) && (s2.pending || done == c2.frags) && c2.consumed <= len;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    const size_t page = (size_t)sysconf(_SC_PAGESIZE);
    for (uint32_t ci = 0; ci < count; ++ci) {
        uint32_t h[6];
        if (fread(h, 4, 6, f) != 6) return 2;
        const State st{h[0], (int32_t)h[1], h[2], h[3]};
        const uint32_t clen = h[4], len = h[5];
        std::vector<uint8_t> w(len);
        if (len && fread(w.data(), 1, len, f) != len) return 2;
        // the reference placement: the checking accessor, the connection 5 bytes into a blob, 9 poison bytes, the carry
        std::vector<uint8_t> blob(5 + (size_t)len + 9 + clen + 3, 0xFF);
        if (len) memcpy(blob.data() + 5, w.data(), len);
        long oob = 0;
        const Checked acc{blob.data(), 5u, 5u + len, &oob};
        Answer ref;
        const uint32_t rc = 5u + len + 9u;
        if (!both(acc, 5u, len, st, rc, clen, &ref)) {
            ++g_bad;
            printf("# case %u: the count pass and the emit pass disagree\n", ci);
        }
        if (oob) {
            ++g_bad;
            printf("# case %u: %ld reads outside the connection\n", ci, oob);
        }
        // plain pointers, the blob ending at a page without access
        const size_t pages = (16u + (size_t)clen + 16u + (size_t)len + 16u + page - 1u) / page + 1u;
        uint8_t* m = (uint8_t*)mmap(nullptr, pages * page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m == MAP_FAILED) return 2;
        if (mprotect(m + (pages - 1u) * page, page, PROT_NONE)) return 2;
        uint8_t* wall = m + (pages - 1u) * page;  // the first byte without access
        for (uint32_t tail : {0u, 11u}) {         // bytes of the blob after the connection (poison)
            for (uint32_t al = 0; al < 4u; ++al) {
                uint8_t* wend = wall - tail;
                uint8_t* wbeg = wend - len;
                const uint32_t shift = (uint32_t)(((uintptr_t)wbeg - al) & 3u);
                wbeg -= shift;
                wend -= shift;
                memset(m, 0xFF, (pages - 1u) * page);
                if (len) memcpy(wbeg, w.data(), len);
                // the blob: 3 + al bytes, the carry window (poison), 2 bytes, the connection, the tail
                uint8_t* base = wbeg - 2u - clen - 3u - al;
                const uint32_t a = (uint32_t)(wbeg - base), cap = a + len + tail, co = 3u + al;
                // (the bytes between the blob's end and the wall are readable: they differ from the poison inside
                // the blob, so that reading them changes the answer)
                for (uint8_t* q = base + cap; q < wall; ++q) *q = 0x00;
                Answer got;
                if (!both((const uint8_t*)base, a, len, st, co, clen, &got) || !same(ref, 5u, rc, got, a, co, len, st.pending != 0)) {
                    ++g_bad;
                    printf("# case %u: alignment %u tail %u disagrees: %u blocks %u fragments\n", ci, al, tail, got.n.blocks, got.n.frags);
                }
            }
        }
        munmap(m, pages * page);
        printf("%u %u %u %u %d %u %u", ref.n.blocks, ref.n.frags, ref.n.open, ref.n.consumed, ref.s.error, ref.s.pending, ref.s.pend_stream);
        for (const Blk& b : ref.c.blocks) printf(" %u %u %u", b.sid_es, b.first, b.nfrag);
        for (size_t i = 0; i < ref.c.frags.size(); ++i) {
            const bool carry = st.pending && i == 0;
            printf(" %u %u", carry ? len : ref.c.frags[i].off - 5u, ref.c.frags[i].len);
        }
        printf("\n");
    }
    fclose(f);
    printf("%s: %ld failures in %u cases\n", g_bad ? "FAILED" : "ok", g_bad, count);
    return g_bad ? 1 : 0;
}
