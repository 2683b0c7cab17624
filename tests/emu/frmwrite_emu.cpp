// host replay of the frame write kernel (loona_amd/csrc/hpk_frmwrite.hip): the REAL per-thread functions of
// hpk_frmwrite.h (fw_elem, fw_chunk, fw_piece, fw_header_octet) and the pack's chunk helpers they share, driven tile
// by tile the way the kernel drives them (a workgroup's contiguous run of tiles, its window of staged blocks restaged
// when used up). The staged arrays are read through a checking accessor, the source blob ends at a page without
// access (to the dword that holds its last octet, as the kernel's loads are), the destination is allocated to the
// byte inside canaries, so a build with -fsanitize=address,undefined also catches any access out of range.
//   frmwrite_emu sweep           M = 1..40, L = 0..3M + 2, every destination and source alignment 0..15, between two
//                                neighbour blocks, against a plain frame-by-frame writer
//   frmwrite_emu file <path>     batches from a file (tests/test_frmwrite_emulation.py writes it): per batch the wire
//                                offsets, the statuses and the octets, for the test to compare with its model
//   frmwrite_emu plain <path>    the same file through the sweep's plain writer alone (no capacity cut): the test holds
//                                it to the same model, so the sweep's answers are the pinned ones
//   frmwrite_emu elems <path>    (block_off[b], block_off[b+1], max_frame, cap) records: the scan's element, the
//                                64-bit running sum and whether it passes HPK_MAX_OFFSET
#include "shim.h"
#include "hpk_frmwrite.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>

#include <random>
#include <string>
#include <vector>

#include "../../include/hpk.h"

using namespace hpkfw;
using hpkpack::pack_chunk_range;
using hpkpack::pack_store;
using hpkpack::pack_upper;

static long g_bad = 0, g_cases = 0, g_oob = 0;

// a staged array: every index is checked
struct Chk {
    const uint32_t* p;
    uint32_t n;
    uint32_t operator[](uint32_t i) const {
        if (i >= n) {
            ++g_oob;
            return 0u;
        }
        return p[i];
    }
};

// The source: `cap` octets at misalignment `mis`, placed so that the dword holding the last octet ends at a page
// with no access.
struct Source {
    uint8_t* map = nullptr;
    size_t map_bytes = 0, page = 0;
    Source() {
        page = (size_t)sysconf(_SC_PAGESIZE);
        map_bytes = page * 64;
        map = (uint8_t*)mmap(nullptr, map_bytes + page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (map == MAP_FAILED || mprotect(map + map_bytes, page, PROT_NONE)) abort();
    }
    // -> the base the kernel's PackSrc gets (the blob starts mis octets in)
    const uint32_t* place(const uint8_t* bytes, uint32_t cap, uint32_t mis) {
        const size_t span = ((size_t)mis + cap + 3u) & ~(size_t)3u;
        if (span > map_bytes) abort();
        uint8_t* base = map + map_bytes - span;
        memset(base, 0xCD, span);
        if (cap) memcpy(base + mis, bytes, cap);
        return (const uint32_t*)base;
    }
};
static Source g_src;

struct Batch {
    std::vector<uint32_t> block_off, sid, mf;  // n + 1, n, n
    std::vector<uint8_t> src;                  // src_cap octets
    uint32_t src_mis = 0, dst_mis = 0, grid = 1;
    int64_t cap_req = -1;  // the destination capacity, -1: the total
};

struct Result {
    std::vector<uint32_t> wire_off;
    std::vector<uint8_t> status, out;  // out: the destination's [0, cap)
    bool void_all = false;
};

static Result run_batch(const char* what, const Batch& B) {
    ++g_cases;
    Result R;
    const uint32_t n = (uint32_t)B.sid.size(), src_cap = (uint32_t)B.src.size();
    // the length scan's rule over the real element
    uint64_t sum = 0;
    std::vector<uint64_t> at(n + 1, 0);
    for (uint32_t b = 0; b < n; ++b) {
        at[b] = sum;
        sum += fw_elem(B.block_off[b], B.block_off[b + 1], B.mf[b], src_cap);
    }
    at[n] = sum;
    R.void_all = sum > (uint64_t)HPK_MAX_OFFSET;
    R.wire_off.assign(n + 1, 0);
    R.status.assign(n, 0);
    for (uint32_t b = 0; b <= n; ++b) R.wire_off[b] = R.void_all ? 0u : (uint32_t)at[b];
    for (uint32_t b = 0; b < n; ++b)
        R.status[b] = (!R.void_all && fw_block_ok(B.block_off[b], B.block_off[b + 1], B.mf[b], src_cap)) ? HPK_OK : HPK_BAD_OFFSETS;
    const uint32_t total = R.wire_off[n];
    const uint32_t dst_cap = B.cap_req < 0 ? total : (uint32_t)B.cap_req;
    const uint32_t limit = total < dst_cap ? total : dst_cap;
    const PackSrc ps{g_src.place(B.src.data(), src_cap, B.src_mis), B.src_mis, src_cap};
    // the destination: 16 canary bytes, the misalignment, the capacity, to the byte
    const uint32_t dst_mis = B.dst_mis;
    const size_t dst_bytes = 16u + dst_mis + (size_t)dst_cap;
    uint8_t* dst_alloc = nullptr;
    if (posix_memalign((void**)&dst_alloc, 16, dst_bytes)) abort();
    memset(dst_alloc, 0xA5, dst_bytes);
    uint8_t* dst_base = dst_alloc + 16;  // what the kernel gets: the blob's address rounded down
    if (limit && n) {
        const uint64_t end = (uint64_t)dst_mis + limit;
        const uint64_t ntiles = (end + kFwTile - 1u) / kFwTile;
        const uint64_t per = (ntiles + B.grid - 1u) / B.grid;
        std::vector<uint32_t> sw(kFwLds + 1), sb(kFwLds + 1), sm(kFwLds), si(kFwLds);
        for (uint32_t wg = 0; wg < B.grid; ++wg) {
            const uint64_t t_first = (uint64_t)wg * per, t_last = t_first + per < ntiles ? t_first + per : ntiles;
            if (t_first >= t_last) continue;
            const uint64_t c_first = t_first * kFwTile;
            uint32_t win_a =
                pack_upper(Chk{R.wire_off.data(), n + 1u}, n + 1u, (uint32_t)((c_first > dst_mis ? c_first : dst_mis) - dst_mis)) - 1u;
            uint32_t win_cnt = 0;
            for (uint64_t t = t_first; t < t_last; ++t) {
                const uint64_t c0 = t * kFwTile, c1 = c0 + kFwTile;
                const uint32_t thi = (uint32_t)((c1 < end ? c1 : end) - dst_mis);
                uint32_t cur = (uint32_t)((c0 > dst_mis ? c0 : dst_mis) - dst_mis);
                static uint32_t acc[kFwThreads][4];
                memset(acc, 0, sizeof acc);
                while (cur < thi) {
                    if (win_cnt == 0u || sw[win_cnt] <= cur) {
                        win_a += win_cnt;
                        if (win_a >= n) {
                            ++g_bad;
                            printf("%s: the window ran past the blocks\n", what);
                            break;
                        }
                        win_cnt = n - win_a < kFwLds ? n - win_a : kFwLds;
                        for (uint32_t j = 0; j <= win_cnt; ++j) sw[j] = R.wire_off[win_a + j], sb[j] = B.block_off[win_a + j];
                        for (uint32_t j = 0; j < win_cnt; ++j) sm[j] = B.mf[win_a + j], si[j] = B.sid[win_a + j];
                    }
                    const uint32_t we = sw[win_cnt], rend = we < thi ? we : thi;
                    for (uint32_t tid = 0; tid < kFwThreads; ++tid) {
                        if (c0 + 16u * (uint64_t)tid >= end) break;
                        uint32_t clo = 0, chi = 0;
                        if (!pack_chunk_range(c0, tid, dst_mis, end, &clo, &chi)) continue;
                        const uint32_t lo = clo > cur ? clo : cur, hi = chi < rend ? chi : rend;
                        if (lo < hi)
                            fw_chunk(acc[tid], Chk{sw.data(), win_cnt + 1u}, Chk{sb.data(), win_cnt + 1u}, Chk{sm.data(), win_cnt},
                                     Chk{si.data(), win_cnt}, win_cnt, lo, hi, (lo + dst_mis) & 15u, ps);
                    }
                    cur = rend > cur ? rend : cur;
                }
                for (uint32_t tid = 0; tid < kFwThreads; ++tid) {
                    if (c0 + 16u * (uint64_t)tid >= end) break;
                    uint32_t clo = 0, chi = 0;
                    if (!pack_chunk_range(c0, tid, dst_mis, end, &clo, &chi)) continue;
                    pack_store(dst_base + c0 + 16u * tid, acc[tid], (clo + dst_mis) & 15u, chi - clo);
                }
            }
        }
    }
    // nothing outside [0, limit) of the blob is touched
    for (size_t i = 0; i < 16u + dst_mis; ++i)
        if (dst_alloc[i] != 0xA5) { ++g_bad; printf("%s: canary before the blob hit at %zu\n", what, i); break; }
    for (size_t i = 16u + dst_mis + limit; i < dst_bytes; ++i)
        if (dst_alloc[i] != 0xA5) { ++g_bad; printf("%s: octet past the limit written at %zu\n", what, i - 16u - dst_mis); break; }
    R.out.assign(dst_alloc + 16u + dst_mis, dst_alloc + 16u + dst_mis + dst_cap);
    free(dst_alloc);
    return R;
}

// the plain writer: server.rs:470-508 frame by frame, lib.rs:413-422 octet by octet
static void plain_write(std::vector<uint8_t>& o, const uint8_t* p, uint32_t L, uint32_t sid, uint32_t M) {
    bool first = true;
    for (;;) {
        const bool last = L <= M;
        const uint32_t n = last ? L : M;
        const uint8_t flags = (uint8_t)((last ? 4 : 0) | (first && (sid >> 31) ? 1 : 0));
        const uint32_t id = sid & 0x7FFFFFFFu;
        const uint8_t h[9] = {(uint8_t)(n >> 16), (uint8_t)(n >> 8), (uint8_t)n, (uint8_t)(first ? 1 : 9), flags,
                              (uint8_t)(id >> 24), (uint8_t)(id >> 16), (uint8_t)(id >> 8), (uint8_t)id};
        o.insert(o.end(), h, h + 9);
        o.insert(o.end(), p, p + n);
        p += n;
        L -= n;
        first = false;
        if (last) return;
    }
}

static int sweep() {
    std::mt19937 rng(7);
    for (uint32_t M = 1; M <= 40; ++M)
        for (uint32_t L = 0; L <= 3 * M + 2; ++L) {
            // the block between two neighbours of other frame sizes, behind a few filler octets
            const uint32_t pre = rng() % 23, post = rng() % 23, base = rng() % 5;
            const uint32_t Mp = 1 + rng() % 9, Mq = 1 + rng() % 30;
            Batch B;
            B.block_off = {base, base + pre, base + pre + L, base + pre + L + post};
            B.sid = {(uint32_t)rng(), (uint32_t)rng(), (uint32_t)rng()};
            B.mf = {Mp, M, Mq};
            B.src.resize(base + pre + L + post);
            for (auto& x : B.src) x = (uint8_t)rng();
            std::vector<uint8_t> want;
            for (int b = 0; b < 3; ++b) plain_write(want, B.src.data() + B.block_off[b], B.block_off[b + 1] - B.block_off[b], B.sid[b], B.mf[b]);
            for (uint32_t dm = 0; dm < 16; ++dm)
                for (uint32_t sm = 0; sm < 16; ++sm) {
                    B.dst_mis = dm;
                    B.src_mis = sm;
                    B.grid = 1 + (dm + sm) % 3;
                    const Result R = run_batch("sweep", B);
                    if (R.out != want) {
                        size_t k = 0;
                        while (k < want.size() && k < R.out.size() && R.out[k] == want[k]) ++k;
                        if (g_bad < 20) printf("sweep M %u L %u dst_mis %u src_mis %u: first difference at wire offset %zu\n", M, L, dm, sm, k);
                        ++g_bad;
                    }
                }
        }
    return 0;
}

static bool read_u32(FILE* f, uint32_t* v, size_t n) { return fread(v, 4, n, f) == n; }

static int from_file(const char* path, bool plain) {
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    uint32_t nb = 0;
    if (!read_u32(f, &nb, 1)) return 2;
    for (uint32_t k = 0; k < nb; ++k) {
        uint32_t h[6];  // n, src_mis, dst_mis, capacity (0xFFFFFFFF: the total), grid, src_cap
        if (!read_u32(f, h, 6)) return 2;
        Batch B;
        const uint32_t n = h[0];
        B.src_mis = h[1], B.dst_mis = h[2], B.cap_req = h[3] == 0xFFFFFFFFu ? -1 : (int64_t)h[3], B.grid = h[4];
        B.block_off.resize(n + 1), B.sid.resize(n), B.mf.resize(n), B.src.resize(h[5]);
        if (!read_u32(f, B.block_off.data(), n + 1) || (n && (!read_u32(f, B.sid.data(), n) || !read_u32(f, B.mf.data(), n)))) return 2;
        if (h[5] && fread(B.src.data(), 1, h[5], f) != h[5]) return 2;
        if (plain) {  // every writable block as the sweep's oracle writes it
            ++g_cases;
            std::vector<uint8_t> o;
            for (uint32_t b = 0; b < n; ++b)
                if (fw_block_ok(B.block_off[b], B.block_off[b + 1], B.mf[b], h[5]))
                    plain_write(o, B.src.data() + B.block_off[b], B.block_off[b + 1] - B.block_off[b], B.sid[b], B.mf[b]);
            printf("P ");
            for (uint8_t v : o) printf("%02x", v);
            printf("\n");
            continue;
        }
        const Result R = run_batch("file", B);
        printf("O");
        for (uint32_t v : R.wire_off) printf(" %u", v);
        printf("\nS");
        for (uint8_t v : R.status) printf(" %u", v);
        printf("\nX ");
        for (uint8_t v : R.out) printf("%02x", v);
        printf("\n");
    }
    fclose(f);
    return 0;
}

static int elems(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    uint32_t n = 0;
    if (!read_u32(f, &n, 1)) return 2;
    uint64_t sum = 0;
    for (uint32_t k = 0; k < n; ++k) {
        uint32_t q[4];
        if (!read_u32(f, q, 4)) return 2;
        const uint64_t w = fw_elem(q[0], q[1], q[2], q[3]);
        sum += w;
        printf("E %llu %llu %d\n", (unsigned long long)w, (unsigned long long)sum, sum > (uint64_t)HPK_MAX_OFFSET ? 1 : 0);
        ++g_cases;
    }
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "sweep";
    int rc = 0;
    if (mode == "sweep") rc = sweep();
    else if ((mode == "file" || mode == "plain") && argc > 2) rc = from_file(argv[2], mode == "plain");
    else if (mode == "elems" && argc > 2) rc = elems(argv[2]);
    else rc = 2;
    if (rc) {
        printf("FAILED: bad arguments or case file\n");
        return rc;
    }
    g_bad += g_oob;
    printf("%s: %ld mismatches in %ld cases (%ld staged reads out of range)\n", g_bad ? "FAILED" : "ok", g_bad, g_cases, g_oob);
    return g_bad ? 1 : 0;
}
