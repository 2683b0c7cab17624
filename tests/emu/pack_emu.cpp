// host replay of the ordered pack kernel (loona_amd/csrc/hpk_pack.hip): the REAL per-thread functions of
// hpk_pack.h (pack_upper, pack_segment, pack_chunk, pack_chunk_range, pack_store), driven tile by tile
// the way the kernel drives them (a workgroup's contiguous run of tiles, its window of staged offsets
// restaged when used up), on layouts that put literal boundaries on and around the tile and window
// edges, with misaligned bases and capacity cuts. The result is compared with memcpy and every byte
// outside the written range with a canary. Source and destination are allocated to the byte, so a build
// with -fsanitize=address,undefined also catches any read or write out of range.
//   usage: pack_emu <seed> <rounds>
#include "shim.h"
#include "hpk_pack.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

using namespace hpkpack;

static long g_bad = 0, g_cases = 0;

struct Layout {
    std::vector<uint32_t> len, src_off;  // n literals
    uint32_t src_cap = 0;
};

// literals of the given lengths at gapped source regions in a shuffled order
static Layout make_layout(const std::vector<uint32_t>& len, std::mt19937& rng, bool shuffle) {
    Layout L;
    L.len = len;
    const size_t n = len.size();
    std::vector<uint32_t> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
    if (shuffle) std::shuffle(order.begin(), order.end(), rng);
    L.src_off.assign(n, 0);
    uint32_t at = rng() % 7;
    for (size_t k = 0; k < n; ++k) {
        const uint32_t i = order[k];
        L.src_off[i] = at;
        at += len[i] + (shuffle ? rng() % 9 : (0u - len[i]) & 3u);  // (in order: 4-aligned starts, as a region layout)
    }
    L.src_cap = at;
    return L;
}

static void run_case(const char* what, const Layout& L, uint32_t src_mis, uint32_t dst_mis, int64_t cap_req, uint32_t grid,
                     std::mt19937& rng) {
    ++g_cases;
    const uint32_t n = (uint32_t)L.len.size();
    std::vector<uint32_t> dst_off(n + 1, 0);
    for (uint32_t i = 0; i < n; ++i) dst_off[i + 1] = dst_off[i] + L.len[i];
    const uint32_t total = dst_off[n];
    const uint32_t dst_cap = cap_req < 0 ? total : (uint32_t)cap_req;
    const uint32_t limit = total < dst_cap ? total : dst_cap;
    // the source, allocated to the last dword that holds a byte of it
    const size_t src_bytes = ((size_t)src_mis + L.src_cap + 3u) & ~(size_t)3u;
    uint8_t* src_alloc = nullptr;
    if (posix_memalign((void**)&src_alloc, 16, src_bytes ? src_bytes : 4)) abort();
    for (size_t i = 0; i < src_bytes; ++i) src_alloc[i] = (uint8_t)rng();
    const uint8_t* src = src_alloc + src_mis;
    // the destination: 16 canary bytes, the misalignment, the capacity, to the byte
    const size_t dst_bytes = 16u + dst_mis + (size_t)dst_cap;
    uint8_t* dst_alloc = nullptr;
    if (posix_memalign((void**)&dst_alloc, 16, dst_bytes)) abort();
    memset(dst_alloc, 0xA5, dst_bytes);
    uint8_t* dst_base = dst_alloc + 16;  // what the kernel gets: the blob's address rounded down
    std::vector<uint8_t> want(dst_bytes, 0xA5);
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t b = 0; b < L.len[i]; ++b)
            if (dst_off[i] + b < limit) want[16u + dst_mis + dst_off[i] + b] = src[L.src_off[i] + b];

    const PackSrc ps{(const uint32_t*)src_alloc, src_mis, L.src_cap};
    if (limit) {
        const uint64_t end = (uint64_t)dst_mis + limit;
        const uint64_t ntiles = (end + kPackTile - 1u) / kPackTile;
        const uint64_t per = (ntiles + grid - 1u) / grid;
        std::vector<uint32_t> sd(kPackLds + 1), ss(kPackLds);
        for (uint32_t wg = 0; wg < grid; ++wg) {
            const uint64_t t_first = (uint64_t)wg * per, t_last = t_first + per < ntiles ? t_first + per : ntiles;
            if (t_first >= t_last) continue;
            const uint64_t c_first = t_first * kPackTile;
            uint32_t win_a = pack_upper(dst_off.data(), n + 1u, (uint32_t)((c_first > dst_mis ? c_first : dst_mis) - dst_mis)) - 1u;
            uint32_t win_cnt = 0;
            for (uint64_t t = t_first; t < t_last; ++t) {
                const uint64_t c0 = t * kPackTile, c1 = c0 + kPackTile;
                const uint32_t thi = (uint32_t)((c1 < end ? c1 : end) - dst_mis);
                uint32_t cur = (uint32_t)((c0 > dst_mis ? c0 : dst_mis) - dst_mis);
                static uint32_t acc[kPackThreads][4];
                memset(acc, 0, sizeof acc);
                while (cur < thi) {
                    if (win_cnt == 0u || sd[win_cnt] <= cur) {
                        win_a += win_cnt;
                        if (win_a >= n) { ++g_bad; printf("%s: window ran past the literals\n", what); break; }
                        win_cnt = n - win_a < kPackLds ? n - win_a : kPackLds;
                        for (uint32_t j = 0; j <= win_cnt; ++j) sd[j] = dst_off[win_a + j];
                        for (uint32_t j = 0; j < win_cnt; ++j) ss[j] = L.src_off[win_a + j];
                    }
                    const uint32_t we = sd[win_cnt], rend = we < thi ? we : thi;
                    for (uint32_t tid = 0; tid < kPackThreads; ++tid) {
                        uint32_t clo = 0, chi = 0;
                        if (!pack_chunk_range(c0, tid, dst_mis, end, &clo, &chi)) continue;
                        const uint32_t lo = clo > cur ? clo : cur, hi = chi < rend ? chi : rend;
                        if (lo < hi) pack_chunk(acc[tid], sd.data(), ss.data(), win_cnt, lo, hi, (lo + dst_mis) & 15u, ps);
                    }
                    cur = rend > cur ? rend : cur;
                }
                for (uint32_t tid = 0; tid < kPackThreads; ++tid) {
                    uint32_t clo = 0, chi = 0;
                    if (!pack_chunk_range(c0, tid, dst_mis, end, &clo, &chi)) continue;
                    pack_store(dst_base + c0 + 16u * tid, acc[tid], (clo + dst_mis) & 15u, chi - clo);
                }
            }
        }
    }
    if (memcmp(dst_alloc, want.data(), dst_bytes) != 0) {
        size_t at = 0;
        while (dst_alloc[at] == want[at]) ++at;
        printf("%s (n %u total %u cap %u src_mis %u dst_mis %u grid %u): first difference at blob offset %ld\n", what, n, total,
               dst_cap, src_mis, dst_mis, grid, (long)at - 16 - (long)dst_mis);
        ++g_bad;
    }
    free(src_alloc);
    free(dst_alloc);
}

static void shorts(std::vector<uint32_t>& v, std::mt19937& rng, int k) {
    for (int i = 0; i < k; ++i) v.push_back(rng() % 40);
}

int main(int argc, char** argv) {
    const uint32_t seed = argc > 1 ? (uint32_t)atoi(argv[1]) : 1u;
    const int rounds = argc > 2 ? atoi(argv[2]) : 2;
    std::mt19937 rng(seed);
    const uint32_t T = kPackTile, Ld = kPackLds;
    for (int r = 0; r < rounds; ++r) {
        std::vector<std::pair<const char*, std::vector<uint32_t>>> cases;
        {   std::vector<uint32_t> v; shorts(v, rng, 5); for (int i = 0; i < 13; ++i) v.push_back(T / 4); shorts(v, rng, 5);
            cases.push_back({"quarter tiles", v}); }
        {   std::vector<uint32_t> v(12, T / 4); cases.push_back({"quarter tiles on the edges", v}); }
        {   std::vector<uint32_t> v; shorts(v, rng, 30); v.push_back(3 * T + 5); shorts(v, rng, 30);
            cases.push_back({"3T+5 mid-tile", v}); }
        {   std::vector<uint32_t> v; shorts(v, rng, 20); v.insert(v.end(), Ld + 1000, 0u); shorts(v, rng, 20);
            cases.push_back({"L+1000 empties", v}); }
        {   std::vector<uint32_t> v; shorts(v, rng, 20); v.insert(v.end(), 2 * Ld, 1u); shorts(v, rng, 20);
            cases.push_back({"2L one-byte", v}); }
        for (uint32_t tot : {2 * T, 2 * T - 1, 2 * T + 1, 17u}) {
            std::vector<uint32_t> v;
            uint32_t left = tot;
            while (left) { const uint32_t x = std::min<uint32_t>(left, 1 + rng() % 200); v.push_back(x); left -= x; }
            cases.push_back({"exact total", v});
        }
        cases.push_back({"all empty", std::vector<uint32_t>(300, 0u)});
        cases.push_back({"n = 1", std::vector<uint32_t>(1, 1 + rng() % 100)});
        cases.push_back({"n = 0", std::vector<uint32_t>()});
        {   std::vector<uint32_t> v; for (int i = 0; i < 3000; ++i) v.push_back(rng() % 8 ? rng() % 70 : rng() % 3000);
            cases.push_back({"random", v}); }
        for (auto& c : cases) {
            const Layout L = make_layout(c.second, rng, true), R = make_layout(c.second, rng, false);
            uint32_t total = 0;
            for (uint32_t x : c.second) total += x;
            for (uint32_t dm : {0u, 1u, 5u, 15u}) {
                const uint32_t sm = rng() % 16;
                run_case(c.first, L, sm, dm, -1, 1 + rng() % 5, rng);
                run_case(c.first, R, (sm + 3) & 15, dm, -1, 1 + rng() % 64, rng);
            }
            // capacity cuts
            for (int64_t cap : {(int64_t)total - 1, (int64_t)T + 3, (int64_t)0, (int64_t)(total ? rng() % total : 0)})
                if (cap >= 0) run_case(c.first, L, rng() % 16, rng() % 16, cap, 1 + rng() % 7, rng);
        }
    }
    printf("%s: %ld mismatches in %ld cases\n", g_bad ? "FAILED" : "ok", g_bad, g_cases);
    return g_bad ? 1 : 0;
}
