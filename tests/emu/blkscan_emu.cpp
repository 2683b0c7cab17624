// host replay of the header-block scan's two passes (loona_amd/csrc/hpk_blkscan.hip): the REAL per-lane walk of
// hpk_blkscan.h (walk_block), one block at a time, on blocks read from a file that tests/test_blkscan_emulation.py
// writes (and whose answers it takes from blocks_scan_cases.ref_scan).
//
// Every block is walked in several placements, which must all agree:
//   * the count pass (the visitor that does nothing) and the emit pass (a visitor that collects) through a checking
//     accessor that counts any index outside the block, the block 5 bytes into a blob with poison on both sides:
//     the counts must be the collected sizes;
//   * both passes through a plain pointer with the blob at the end of a buffer whose next page has no access, the
//     block at each of the 4 dword alignments, once ending with the blob and once followed inside the blob by
//     poison bytes (0xFF: an indexed field, and a continuation octet), so a read past the block changes the answer
//     or faults.
//   usage: blkscan_emu <cases file>      file: u32 count, then per case u32 length + the block's bytes
//   output: one line per case: nfields nstrs, then per field index str kind nstr err err_stage at, then per
//   string off end (offsets relative to the block)
#include "shim.h"
#include "hpk_blkscan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>

#include <utility>
#include <vector>

using namespace hpkblk;

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

struct Collect {
    std::vector<hpk_field> fields;
    std::vector<std::pair<uint32_t, uint32_t>> strs;
    long order_bad = 0;
    void field(uint32_t i, const hpk_field& f) {
        if (i != fields.size() || f.str + f.nstr != strs.size()) ++order_bad;
        fields.push_back(f);
    }
    void string(uint32_t s, uint32_t off, uint32_t end) {
        if (s != strs.size()) ++order_bad;
        strs.push_back({off, end});
    }
};

// (offsets relative to each walk's block start)
static bool same(const Collect& x, uint32_t dx, const Collect& y, uint32_t dy) {
    if (x.fields.size() != y.fields.size() || x.strs.size() != y.strs.size()) return false;
    for (size_t i = 0; i < x.fields.size(); ++i) {
        const hpk_field &a = x.fields[i], &b = y.fields[i];
        if (a.index != b.index || a.str != b.str || a.kind != b.kind || a.nstr != b.nstr || a.err != b.err ||
            a.err_stage != b.err_stage || a.at - dx != b.at - dy)
            return false;
    }
    for (size_t i = 0; i < x.strs.size(); ++i)
        if (x.strs[i].first - dx != y.strs[i].first - dy || x.strs[i].second - dx != y.strs[i].second - dy) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    const size_t page = (size_t)sysconf(_SC_PAGESIZE);
    for (uint32_t ci = 0; ci < count; ++ci) {
        uint32_t len = 0;
        if (fread(&len, 4, 1, f) != 1) return 2;
        std::vector<uint8_t> w(len);
        if (len && fread(w.data(), 1, len, f) != len) return 2;
        // the reference placement: the checking accessor, the block 5 bytes into a blob with 9 bytes after it
        std::vector<uint8_t> blob(5 + (size_t)len + 9, 0xFF);
        if (len) memcpy(blob.data() + 5, w.data(), len);
        long oob = 0;
        const Checked acc{blob.data(), 5u, 5u + len, &oob};
        NoVisit nv;
        const Counts cnt = walk_block(acc, 5u, 5u + len, nv);
        Collect ref;
        const Counts cnt2 = walk_block(acc, 5u, 5u + len, ref);
        if (oob) { ++g_bad; printf("# case %u: %ld reads outside the block\n", ci, oob); }
        if (cnt.fields != ref.fields.size() || cnt.strs != ref.strs.size() || cnt2.fields != cnt.fields || cnt2.strs != cnt.strs ||
            ref.order_bad) {
            ++g_bad;
            printf("# case %u: the count pass (%u, %u) and the emit pass (%zu, %zu) disagree\n", ci, cnt.fields, cnt.strs,
                   ref.fields.size(), ref.strs.size());
        }
        // plain pointers, the blob ending at a page without access
        const size_t pages = (16u + (size_t)len + 16u + page - 1u) / page + 1u;
        uint8_t* m = (uint8_t*)mmap(nullptr, pages * page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m == MAP_FAILED) return 2;
        if (mprotect(m + (pages - 1u) * page, page, PROT_NONE)) return 2;
        uint8_t* wall = m + (pages - 1u) * page;  // the first byte without access
        for (uint32_t tail : {0u, 7u}) {          // bytes of the blob after the block (poison)
            for (uint32_t al = 0; al < 4u; ++al) {
                // the block's first byte at dword alignment al: the blob's end moves back by up to 3 bytes
                uint8_t* wend = wall - tail;
                uint8_t* wbeg = wend - len;
                const uint32_t shift = (uint32_t)(((uintptr_t)wbeg - al) & 3u);
                wbeg -= shift;
                wend -= shift;
                memset(m, 0xFF, (pages - 1u) * page);
                if (len) memcpy(wbeg, w.data(), len);
                uint8_t* base = wbeg - 3u - al;
                const uint32_t a = (uint32_t)(wbeg - base), e = a + len, cap = e + tail;
                // (the bytes between the blob's end and the wall are readable: they differ from the poison inside
                // the blob, so that reading them changes the answer)
                for (uint8_t* q = base + cap; q < wall; ++q) *q = 0x00;
                NoVisit nv2;
                const Counts c = walk_block((const uint8_t*)base, a, e, nv2);
                Collect got;
                (void)walk_block((const uint8_t*)base, a, e, got);
                if (c.fields != cnt.fields || c.strs != cnt.strs || !same(ref, 5u, got, a)) {
                    ++g_bad;
                    printf("# case %u: alignment %u tail %u disagrees: %u fields %u strings\n", ci, al, tail, c.fields, c.strs);
                }
            }
        }
        munmap(m, pages * page);
        printf("%zu %zu", ref.fields.size(), ref.strs.size());
        for (const hpk_field& x : ref.fields)
            printf(" %u %u %u %u %u %u %u", x.index, x.str, x.kind, x.nstr, x.err, x.err_stage, x.at - 5u);
        for (const auto& s : ref.strs) printf(" %u %u", s.first - 5u, s.second - 5u);
        printf("\n");
    }
    fclose(f);
    printf("%s: %ld failures in %u cases\n", g_bad ? "FAILED" : "ok", g_bad, count);
    return g_bad ? 1 : 0;
}
