// host replay of the two-source ordered pack (hpk_pack2, loona_amd/csrc/hpk_decode_strings.hip): the REAL
// per-thread functions of hpk_pack.h (pack2_chunk with pack_upper, pack_segment, pack_chunk_range, pack_store),
// driven tile by tile the way the kernel drives them (a workgroup's contiguous run of tiles, its window of staged
// offsets and selectors restaged when used up). Every literal lies in one of two source blobs, picked at
// random per literal; each blob is allocated to the last dword that holds a byte of it, so a build with
// -fsanitize=address also catches any read out of range, and the bytes of that allocation outside the blob (its
// misaligned lead and the rest of its last dword) are poisoned with a value no literal byte has: a byte taken
// from just outside either source's range shows in the comparison with memcpy. Every destination byte outside the
// written range is compared with a canary.
//   usage: pack2_emu <seed> <rounds>
#include "shim.h"
#include "hpk_pack.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

using namespace hpkpack;

static long g_bad = 0, g_cases = 0, g_mixed_chunks = 0;

static const uint8_t kPoison = 0xEE;  // (literal bytes are 0 .. 0xDF)

struct Source {
    uint8_t* alloc = nullptr;
    uint32_t mis = 0, cap = 0;
    const uint8_t* blob() const { return alloc + mis; }
};

static Source make_source(uint32_t mis, uint32_t cap, std::mt19937& rng) {
    Source s;
    s.mis = mis;
    s.cap = cap;
    const size_t bytes = ((size_t)mis + cap + 3u) & ~(size_t)3u;
    if (posix_memalign((void**)&s.alloc, 16, bytes ? bytes : 4)) abort();
    memset(s.alloc, kPoison, bytes ? bytes : 4);
    for (uint32_t i = 0; i < cap; ++i) s.alloc[mis + i] = (uint8_t)(rng() % 0xE0);
    return s;
}

static void run_case(const char* what, const std::vector<uint32_t>& len, const std::vector<uint8_t>& sel, uint32_t mis0,
                     uint32_t mis1, uint32_t dst_mis, int64_t cap_req, uint32_t grid, std::mt19937& rng) {
    ++g_cases;
    const uint32_t n = (uint32_t)len.size();
    // each source's literals at gapped offsets in a shuffled order; a literal ends exactly at its source's end
    std::vector<uint32_t> src_off(n, 0), order(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    std::shuffle(order.begin(), order.end(), rng);
    uint32_t at[2] = {0, 0};
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t i = order[k], s = sel[i] ? 1u : 0u;
        at[s] += rng() % 5;
        src_off[i] = at[s];
        at[s] += len[i];
    }
    const Source S0 = make_source(mis0, at[0], rng), S1 = make_source(mis1, at[1], rng);
    std::vector<uint32_t> dst_off(n + 1, 0);
    for (uint32_t i = 0; i < n; ++i) dst_off[i + 1] = dst_off[i] + len[i];
    const uint32_t total = dst_off[n];
    const uint32_t dst_cap = cap_req < 0 ? total : (uint32_t)cap_req;
    const uint32_t limit = total < dst_cap ? total : dst_cap;
    const size_t dst_bytes = 16u + dst_mis + (size_t)dst_cap;
    uint8_t* dst_alloc = nullptr;
    if (posix_memalign((void**)&dst_alloc, 16, dst_bytes)) abort();
    memset(dst_alloc, 0xA5, dst_bytes);
    uint8_t* dst_base = dst_alloc + 16;
    std::vector<uint8_t> want(dst_bytes, 0xA5);
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t* src = sel[i] ? S1.blob() : S0.blob();
        for (uint32_t b = 0; b < len[i]; ++b)
            if (dst_off[i] + b < limit) want[16u + dst_mis + dst_off[i] + b] = src[src_off[i] + b];
    }
    // chunks that hold bytes of both sources (the case must have some where it claims to)
    for (uint32_t i = 0; i + 1 < n; ++i)
        if (len[i] && len[i + 1] && sel[i] != sel[i + 1] && dst_off[i + 1] < limit && ((dst_off[i + 1] + dst_mis) & 15u)) ++g_mixed_chunks;

    const PackSrc p0{(const uint32_t*)S0.alloc, S0.mis, S0.cap}, p1{(const uint32_t*)S1.alloc, S1.mis, S1.cap};
    if (limit) {
        const uint64_t end = (uint64_t)dst_mis + limit;
        const uint64_t ntiles = (end + kPackTile - 1u) / kPackTile;
        const uint64_t per = (ntiles + grid - 1u) / grid;
        std::vector<uint32_t> sd(kPackLds + 1), ss(kPackLds);
        std::vector<uint8_t> sx(kPackLds);
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
                        for (uint32_t j = 0; j < win_cnt; ++j) ss[j] = src_off[win_a + j], sx[j] = sel[win_a + j];
                    }
                    const uint32_t we = sd[win_cnt], rend = we < thi ? we : thi;
                    for (uint32_t tid = 0; tid < kPackThreads; ++tid) {
                        uint32_t clo = 0, chi = 0;
                        if (!pack_chunk_range(c0, tid, dst_mis, end, &clo, &chi)) continue;
                        const uint32_t lo = clo > cur ? clo : cur, hi = chi < rend ? chi : rend;
                        if (lo < hi)
                            pack2_chunk(acc[tid], sd.data(), ss.data(), sx.data(), win_cnt, lo, hi, (lo + dst_mis) & 15u, p0, p1);
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
        size_t a = 0;
        while (dst_alloc[a] == want[a]) ++a;
        printf("%s (n %u total %u cap %u mis %u/%u dst_mis %u grid %u): first difference at blob offset %ld: %02x for %02x\n", what,
               n, total, dst_cap, mis0, mis1, dst_mis, grid, (long)a - 16 - (long)dst_mis, dst_alloc[a], want[a]);
        ++g_bad;
    }
    free(S0.alloc);
    free(S1.alloc);
    free(dst_alloc);
}

static void shorts(std::vector<uint32_t>& v, std::mt19937& rng, int k) {
    for (int i = 0; i < k; ++i) v.push_back(rng() % 40);
}

int main(int argc, char** argv) {
    const uint32_t seed = argc > 1 ? (uint32_t)atoi(argv[1]) : 1u;
    const int rounds = argc > 2 ? atoi(argv[2]) : 1;
    std::mt19937 rng(seed);
    const uint32_t T = kPackTile, Ld = kPackLds;
    for (int r = 0; r < rounds; ++r) {
        std::vector<std::pair<const char*, std::vector<uint32_t>>> cases;
        {   std::vector<uint32_t> v; for (int i = 0; i < 3000; ++i) v.push_back(1 + rng() % 7);
            cases.push_back({"1-7 byte literals", v}); }
        {   std::vector<uint32_t> v; shorts(v, rng, 20); v.insert(v.end(), Ld + 1000, 0u); shorts(v, rng, 20);
            cases.push_back({"L+1000 empties", v}); }
        {   std::vector<uint32_t> v; shorts(v, rng, 30); v.push_back(T + 17); shorts(v, rng, 30);
            cases.push_back({"T+17 mid-tile", v}); }
        {   std::vector<uint32_t> v; shorts(v, rng, 10); v.push_back(3 * T + 5); v.push_back(2 * T + 1); shorts(v, rng, 10);
            cases.push_back({"two long neighbours", v}); }
        {   std::vector<uint32_t> v; for (int i = 0; i < 3000; ++i) v.push_back(rng() % 8 ? rng() % 70 : rng() % 3000);
            cases.push_back({"random", v}); }
        cases.push_back({"all empty", std::vector<uint32_t>(300, 0u)});
        cases.push_back({"n = 1", std::vector<uint32_t>(1, 1 + rng() % 100)});
        cases.push_back({"n = 0", std::vector<uint32_t>()});
        for (auto& c : cases) {
            const uint32_t n = (uint32_t)c.second.size();
            uint32_t total = 0;
            for (uint32_t x : c.second) total += x;
            std::vector<uint8_t> rnd(n), alt(n), one(n, 1), zero(n, 0);
            for (uint32_t i = 0; i < n; ++i) rnd[i] = (uint8_t)(rng() & 1u), alt[i] = (uint8_t)(i & 1u);
            // both sources at every misalignment 0..15 (the other's and the destination's random)
            for (uint32_t m = 0; m < 16u; ++m) {
                run_case(c.first, c.second, rnd, m, rng() % 16, rng() % 16, -1, 1 + rng() % 5, rng);
                run_case(c.first, c.second, alt, rng() % 16, m, rng() % 16, -1, 1 + rng() % 64, rng);
            }
            run_case(c.first, c.second, one, 3, 5, 7, -1, 2, rng);
            run_case(c.first, c.second, zero, 3, 5, 7, -1, 2, rng);
            for (int64_t cap : {(int64_t)total - 1, (int64_t)T + 3, (int64_t)0, (int64_t)(total ? rng() % total : 0)})
                if (cap >= 0) run_case(c.first, c.second, rnd, rng() % 16, rng() % 16, rng() % 16, cap, 1 + rng() % 7, rng);
        }
    }
    if (g_mixed_chunks < 1000) { ++g_bad; printf("only %ld chunks mixed both sources\n", g_mixed_chunks); }
    printf("%s: %ld mismatches in %ld cases (%ld chunks with both sources)\n", g_bad ? "FAILED" : "ok", g_bad, g_cases, g_mixed_chunks);
    return g_bad ? 1 : 0;
}
