// host replay of the string-literal decode's parse step (loona_amd/csrc/hpk_decode_strings.hip): the REAL
// per-thread function of hpk_strparse.h (str_parse), one window at a time, on windows read from a file that
// tests/test_strparse_emulation.py writes (and whose answers it takes from hpack_ref).
//
// Every window is parsed in several placements, which must all agree:
//   * through a checking accessor that counts any index outside the window's intersection with the blob;
//   * through a plain pointer with the blob at the end of a buffer whose next page has no access, the window at
//     each of the 4 dword alignments (which moves the blob's end back by up to 3 bytes: those bytes are zeroed,
//     a terminating octet, and anything further faults), once ending with the blob and once followed inside the
//     blob by poison bytes (0xFF: a continuation octet), so a read past the window's end changes the answer;
//   * with the blob's capacity cut to the window's end minus one: the window is void and nothing is read.
//   usage: strparse_emu <cases file>      file: u32 count, then per case u32 length + the window's bytes
//   output: one line per case: status huff start-relative-to-the-window len consumed
#include "shim.h"
#include "hpk_strparse.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>

#include <vector>

using namespace hpkstr;

static long g_bad = 0;

struct Checked {
    const uint8_t* p;
    uint32_t lo, hi;
    mutable long* oob;
    uint8_t operator[](uint32_t i) const {
        if (i < lo || i >= hi) {
            ++*oob;
            return 0xFF;
        }
        return p[i];
    }
};

static bool same(const StrParse& x, const StrParse& y, uint32_t dx, uint32_t dy) {
    if (x.status != y.status || x.huff != y.huff || x.len != y.len || x.consumed != y.consumed) return false;
    return x.status != HPK_OK || x.start - dx == y.start - dy;
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
        // the reference placement: the checking accessor, the window 5 bytes into a blob with 9 bytes after it
        std::vector<uint8_t> blob(5 + (size_t)len + 9, 0xFF);
        if (len) memcpy(blob.data() + 5, w.data(), len);
        long oob = 0;
        const Checked acc{blob.data(), 5u, 5u + len, &oob};
        const StrParse ref = str_parse(acc, (uint32_t)blob.size(), 5u, 5u + len);
        if (oob) { ++g_bad; printf("# case %u: %ld reads outside the window\n", ci, oob); }
        // a window that passes the capacity, and one that ends before it starts: void, nothing read
        oob = 0;
        const Checked none{blob.data(), 0u, 0u, &oob};
        const StrParse v1 = str_parse(none, 5u + len - 1u, 5u, 5u + len);
        const StrParse v2 = str_parse(none, (uint32_t)blob.size(), 5u + len + 1u, 5u + len);
        if (oob || v1.status != HPK_BAD_OFFSETS || v2.status != HPK_BAD_OFFSETS || v1.consumed || v2.len) {
            ++g_bad;
            printf("# case %u: a void window was read or accepted\n", ci);
        }
        // plain pointers, the blob ending at a page without access
        const size_t pages = (16u + (size_t)len + 16u + page - 1u) / page + 1u;
        uint8_t* m = (uint8_t*)mmap(nullptr, pages * page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (m == MAP_FAILED) return 2;
        if (mprotect(m + (pages - 1u) * page, page, PROT_NONE)) return 2;
        uint8_t* wall = m + (pages - 1u) * page;  // the first byte without access
        for (uint32_t tail : {0u, 7u}) {          // bytes of the blob after the window (poison)
            for (uint32_t al = 0; al < 4u; ++al) {
                // the window's first byte at dword alignment al: the blob's end moves back by up to 3 bytes
                uint8_t* wend = wall - tail;
                uint8_t* wbeg = wend - len;
                const uint32_t shift = (uint32_t)(((uintptr_t)wbeg - al) & 3u);
                wbeg -= shift;
                wend -= shift;
                // the blob is [base, wend + tail); what follows it up to the wall is not part of it
                memset(m, 0xFF, (pages - 1u) * page);
                if (len) memcpy(wbeg, w.data(), len);
                uint8_t* base = wbeg - 3u - al;
                const uint32_t a = (uint32_t)(wbeg - base), e = a + len, cap = e + tail;
                // (the bytes between the blob's end and the wall are readable: make them differ from the poison
                // inside the blob, so that reading them changes the answer)
                for (uint8_t* q = base + cap; q < wall; ++q) *q = 0x00;
                const StrParse r = str_parse((const uint8_t*)base, cap, a, e);
                if (!same(ref, r, 5u, a)) {
                    ++g_bad;
                    printf("# case %u: alignment %u tail %u disagrees: status %u len %u consumed %u\n", ci, al, tail, r.status,
                           r.len, r.consumed);
                }
            }
        }
        munmap(m, pages * page);
        printf("%u %u %u %u %u\n", ref.status, ref.huff, ref.status == HPK_OK ? ref.start - 5u : 0u, ref.len, ref.consumed);
    }
    fclose(f);
    printf("%s: %ld failures in %u cases\n", g_bad ? "FAILED" : "ok", g_bad, count);
    return g_bad ? 1 : 0;
}
