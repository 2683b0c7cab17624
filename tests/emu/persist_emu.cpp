// Host emulation of what one lane of the small-call mode's persistent kernel does for one literal, with the REAL
// functions of loona_amd/csrc/hpk_persist_lit.h (persist_literal_lds, persist_literal; tests/emu/shim.h stands in
// for the HIP language), one lane at a time, against the oracle:
//   a. the store plan, exhaustive: every (out_mis + o0) mod 16 x every decoded count 0..180 on the staged bound
//      path (literals of 5-bit codes: 180 of them are 113 bytes): the oracle's bytes in [ob, ob + cnt), every
//      byte outside the literal's region still the sentinel;
//   b. input placement: every (in_mis + p0) mod 16 x lengths 1..113 x the literal mix of tests/test_gpu_tail.py
//      (text, 5-bit-only text, a 13..28-bit code last, bad padding, more than 7 bits of padding, EOS, a code cut
//      by the end, random bytes, and the reference's error vectors from the file given): length, status, bytes;
//   c. independence: every case of b twice, once with 0xFF and once with random bytes around the literal in the
//      input, in the input slot's previous contents and behind the slot;
//   d. short regions: a sample of b's literals at every capacity 0 .. bound - 1 (the code-by-code walk), against
//      the oracle at that capacity;
//   e. the global walker: lengths 114..300 and three of 1-4 KiB at every (out_mis + o0) mod 8 and every
//      (in_mis + p0) mod 16, capacities bound, count, count - 1, count - 2 and 0;
//   f. the dispatch: 113 bytes is staged at every misalignment in at most 8 chunks, 114 bytes never.
// The input slot, the output slot and the two blobs are heap allocations of their own, so the program is also a
// target for a host sanitizer build (-fsanitize=address,undefined). The output slot is exactly kPersistOutDw
// dwords. The input slot is kPersistInStride dwords and kPast more: the lane walk reads up to three dwords past
// its slot (lit12_load and the steps read dwords (X >> 5) + 1 and (X >> 5) + 2, and X >> 5 reaches 33 where a
// literal ends in its eighth chunk's last bytes). In the kernel they are the next lane's pad dword and first two
// input dwords; behind the last lane's slot, whatever LDS array follows s_slot, or nothing, where an LDS read
// returns zero. They only ever supply bits past the literal's end, which the walk never lets decide anything
// (hpk_walk.h, "Bits past a literal's end are never masked"): check c varies them and the results do not move.
// With -DPERSIST_EMU_PAST=0 a sanitizer build stops at the first such read.
// Test infrastructure only (tests/test_persist_emulation.py). Exit status 0 = no mismatch.
#include "shim.h"
#include "hpk_persist_lit.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <utility>
#include <vector>
extern "C" int oracle_decode(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len);
using namespace hpkdec;

#ifndef PERSIST_EMU_PAST
#define PERSIST_EMU_PAST 3
#endif
constexpr uint32_t kPast = PERSIST_EMU_PAST;
constexpr uint8_t kSent = 0xEE;
constexpr int kThreads = 256;

typedef std::vector<uint8_t> Bytes;
static hpk_tables T;
static std::mt19937_64 rng;
static uint32_t rnd(uint32_t n) { return (uint32_t)(rng() % n); }

enum Path { kEmpty, kStagedBound, kStagedBytes, kGlobal, kPaths };
static const char* kPathName[kPaths] = {"empty", "staged_bound", "staged_bytes", "global"};
static long g_paths[kPaths];

// hpk_persist.h, hpk_persist's literal loop, the test under "staged or global" (as a function of the header it
// compiled to other device code, so it is restated here)
static bool staged(uint32_t b0, uint32_t nbytes) {
    return ((b0 + nbytes + 15u) >> 4) - (b0 >> 4) <= kPersistSlotChunks && nbytes <= kPersistSlotMax;
}

// the pieces the store plan of persist_literal_lds uses for cnt bytes at ob (coverage only: the bytes are checked
// against the oracle)
struct Plan { uint32_t head, lead, groups, trail, tail; };
static Plan store_plan(uint32_t ob, uint32_t cnt) {
    const uint32_t e = ob + cnt, h = min((ob + 3u) & ~3u, e), t = max(e & ~3u, h);
    const uint32_t h16 = min((h + 15u) & ~15u, t), t16 = max(t & ~15u, h16);
    return {h - ob, (h16 - h) / 4u, (t16 - h16) / 16u, (t - t16) / 4u, e - t};
}
static long g_piece[5];

static uint32_t* g_islot;  // kPersistInStride + kPast dwords
static uint32_t* g_oslot;  // kPersistOutDw dwords

struct Case {
    const uint8_t* lit;
    uint32_t n;
    uint32_t in_mis, p0, after;  // the literal at in_base + in_mis + p0, `after` bytes of the batch behind it
    uint32_t out_mis, o0, cap;
    int fill;  // around the literal, in the slots and behind the input slot: 0 random bytes, 1 0xFF
};
struct Got {
    uint32_t cnt, st;
    Path path;
    bool clean;  // no byte outside the region changed
    Bytes bytes;
};

static Got run_case(const Case& c) {
    const uint32_t b0 = c.in_mis + c.p0, p1 = c.p0 + c.n, in_end = c.in_mis + p1 + c.after;
    const uint32_t last16 = in_end ? (in_end - 1u) >> 4 : 0u;
    const size_t ibytes = ((size_t)last16 + 1u) * 16u;
    uint8_t* ibuf = (uint8_t*)aligned_alloc(16, ibytes);
    for (size_t j = 0; j < ibytes; ++j) ibuf[j] = c.fill ? 0xFF : (uint8_t)rng();
    if (c.n) memcpy(ibuf + b0, c.lit, c.n);
    const uint32_t ob = c.out_mis + c.o0, o1 = c.o0 + c.cap;
    const size_t obytes = (((size_t)ob + c.cap + 15u) & ~(size_t)15u) + 64u;
    uint8_t* obuf = (uint8_t*)aligned_alloc(16, obytes);
    memset(obuf, kSent, obytes);
    for (uint32_t j = 0; j < kPersistInStride + kPast; ++j) g_islot[j] = c.fill ? 0xFFFFFFFFu : (uint32_t)rng();
    for (uint32_t j = 0; j < kPersistOutDw; ++j) g_oslot[j] = (uint32_t)rng();
    const u32x4* g16 = reinterpret_cast<const u32x4*>(ibuf);
    auto ld16 = [&](uint32_t ci) {
        const u32x4 v = g16[min(ci, last16)];
        return uint4{v.x, v.y, v.z, v.w};
    };
    Got g;
    g.cnt = g.st = 0xFFFFFFFFu;
    if (staged(b0, c.n)) {
        persist_literal_lds<kThreads>(g16, last16, g_islot, reinterpret_cast<uint8_t*>(g_oslot), T.lut3, T.lo, obuf, c.out_mis,
                                      c.in_mis, c.p0, p1, c.o0, o1, g.cnt, g.st);
        g.path = c.n == 0 ? kEmpty : c.cap >= c.n * 8u / 5u ? kStagedBound : kStagedBytes;
    } else {
        persist_literal(ld16, T.lut3, T.lo, obuf, c.out_mis, c.in_mis, c.p0, p1, c.o0, o1, g.cnt, g.st);
        g.path = kGlobal;
    }
    g_paths[g.path] += 1;
    g.clean = true;
    for (size_t j = 0; j < obytes; ++j)
        if ((j < ob || j >= (size_t)ob + c.cap) && obuf[j] != kSent) g.clean = false;
    const uint32_t k = min(g.cnt, c.cap);
    g.bytes.assign(obuf + ob, obuf + ob + k);
    free(ibuf);
    free(obuf);
    return g;
}

// the oracle at a capacity, kept per (literal, capacity): placement does not change it
struct Ref { int st; Bytes bytes; };
static std::map<std::pair<Bytes, uint32_t>, Ref> g_refs;
static const Ref& oracle_at(const Bytes& lit, uint32_t cap, bool keep) {
    static Ref tmp;
    const auto key = std::make_pair(lit, cap);
    if (keep) {
        auto it = g_refs.find(key);
        if (it != g_refs.end()) return it->second;
    }
    Ref r;
    r.bytes.resize(cap + 8u);
    size_t rl = 0;
    r.st = oracle_decode(lit.data(), lit.size(), r.bytes.data(), cap, &rl);
    r.bytes.resize(rl);
    if (keep) return g_refs[key] = r;
    return tmp = r;
}

static long g_shown = 0;
static bool same(const Got& g, const Ref& r, const Case& c, const char* what) {
    const bool ok = g.clean && (int)g.st == r.st && g.cnt == r.bytes.size() && g.bytes == r.bytes;
    if (!ok && g_shown++ < 12)
        printf("%s: %u bytes at in %u+%u out %u+%u cap %u fill %d (%s): status %u for %d, length %u for %zu%s%s\n", what, c.n,
               c.in_mis, c.p0, c.out_mis, c.o0, c.cap, c.fill, kPathName[g.path], g.st, r.st, g.cnt, r.bytes.size(),
               g.clean ? "" : ", a byte outside the region changed",
               g.cnt == r.bytes.size() && g.bytes != r.bytes ? ", bytes differ" : "");
    return ok;
}

// ---- literals of an exact length ----
struct Bits {
    Bytes b;
    uint32_t n = 0;
    void put(uint32_t code, uint32_t len) {
        for (uint32_t i = len; i-- > 0;) {
            if ((n & 7u) == 0u) b.push_back(0);
            b[n >> 3] |= (uint8_t)(((code >> i) & 1u) << (7u - (n & 7u)));
            n += 1u;
        }
    }
    void ones(uint32_t k) { while (k--) put(1u, 1u); }
};
static const char kText[] = "abcdefghijklmnopqrstuvwxyz0123456789-_=;,/.:ABC ";
static const char kFive[] = "012aceiost";
static std::vector<int> g_longs, g_longs30;  // symbols with codes of 13..28 bits, of 13..30 bits
enum Kind { kKText, kKFive, kKLongLast, kKBadPad, kKPad8, kKEos, kKCut, kKRandom, kKinds };

// symbols of `pool` (5-bit ones where the pool's do not fit) until `keep` + r bits are left, r in 0..7; returns r
static uint32_t fill_to(Bits& s, uint32_t tot, uint32_t keep, const char* pool) {
    for (;;) {
        const uint32_t r = tot - s.n - keep;
        if (r < 5u || (r <= 7u && (rng() & 1u))) return r;
        int c = pool[rnd((uint32_t)strlen(pool))];
        if (T.len[c] > r) c = kFive[rnd(10)];
        s.put(T.code[c], T.len[c]);
    }
}

static Bytes make_literal(int kind, uint32_t L) {
    const uint32_t tot = 8u * L;
    Bits s;
    if (kind == kKRandom) {
        Bytes b(L);
        for (auto& x : b) x = (uint8_t)rng();
        return b;
    }
    if (kind == kKText || kind == kKFive) {
        s.ones(fill_to(s, tot, 0, kind == kKFive ? kFive : kText));
    } else if (kind == kKLongLast) {
        const int c = g_longs[rnd((uint32_t)g_longs.size())];
        if (T.len[c] > tot) {
            s.put(T.code[c] >> (T.len[c] - tot), tot);  // (too short for it: the code cut by the end)
        } else {
            const uint32_t r = fill_to(s, tot, T.len[c], kText);
            s.put(T.code[c], T.len[c]);
            s.ones(r);
        }
    } else if (kind == kKBadPad) {
        const uint32_t r = fill_to(s, tot, 0, kText);
        if (r) s.put(rnd(1u << r) & ~1u, r); else s.b[L - 1] &= 0xFE;
    } else if (kind == kKPad8) {
        if (L == 1) s.ones(8); else s.ones(fill_to(s, tot, 8, kText) + 8u);
    } else if (kind == kKEos) {
        if (tot < 30u) {
            s.ones(tot);
        } else {
            fill_to(s, tot, 30u + 8u * rnd((tot - 30u) / 8u + 1u), kText);
            s.ones(30);
            while (s.n < tot) s.put((uint32_t)rng() & 1u, 1);
        }
    } else {  // kKCut: the first bits of a 13..30-bit code at the end, ones before or behind them where bits are left
        const int c = g_longs30[rnd((uint32_t)g_longs30.size())];
        const uint32_t cut = min(1u + rnd(T.len[c] - 1u), tot);
        const uint32_t r = fill_to(s, tot, cut, kText);
        const bool first = rng() & 1u;
        if (!first) s.ones(r);
        s.put(T.code[c] >> (T.len[c] - cut), cut);
        if (first) s.ones(r);
    }
    if (s.n != tot || s.b.size() != L) {
        printf("make_literal(%d, %u) made %u bits\n", kind, L, s.n);
        exit(2);
    }
    return s.b;
}

static std::vector<Bytes> read_vectors(const char* path) {  // u32 count, then per literal u32 bytes and the bytes
    std::vector<Bytes> v;
    FILE* f = fopen(path, "rb");
    if (!f) {
        printf("cannot read %s\n", path);
        exit(2);
    }
    uint32_t n = 0, k = 0;
    if (fread(&n, 4, 1, f) != 1) exit(2);
    for (uint32_t i = 0; i < n; ++i) {
        if (fread(&k, 4, 1, f) != 1) exit(2);
        Bytes b(k);
        if (k && fread(b.data(), 1, k, f) != k) exit(2);
        v.push_back(b);
    }
    fclose(f);
    return v;
}

// out_mis and o0 (>= 16: sentinels in front) with (out_mis + o0) mod 16 == res
static void place_out(Case& c, uint32_t res) {
    c.out_mis = rnd(16);
    c.o0 = 16u + ((res + 32u - c.out_mis) & 15u) + 16u * rnd(3);
}
static void place_in(Case& c, uint32_t res) {
    c.in_mis = rnd(16);
    c.p0 = ((res + 16u - c.in_mis) & 15u) + 16u * rnd(4);
    c.after = rnd(3) ? rnd(40) : 0u;
}

int main(int argc, char** argv) {
    if (hpk_build_tables(&T)) {
        printf("table build failed\n");
        return 1;
    }
    rng.seed(argc > 1 ? atoi(argv[1]) : 1);
    std::vector<Bytes> vectors;
    if (argc > 2 && strcmp(argv[2], "-") != 0) vectors = read_vectors(argv[2]);
    for (int s = 0; s < 256; ++s) {
        if (T.len[s] >= 13 && T.len[s] <= 28) g_longs.push_back(s);
        if (T.len[s] >= 13) g_longs30.push_back(s);
    }
    g_islot = (uint32_t*)malloc((kPersistInStride + kPast) * 4u);
    g_oslot = (uint32_t*)malloc(kPersistOutDw * 4u);
    long bad = 0;

    // a. the store plan
    {
        long cases = 0, a_bad = 0;
        const uint32_t top = kPersistSlotMax * 8u / 5u;  // 180
        for (uint32_t res = 0; res < 16; ++res)
            for (uint32_t count = 0; count <= top; ++count)
                for (int rep = 0; rep < 4; ++rep) {
                    Bits s;
                    for (uint32_t j = 0; j < count; ++j) s.put(T.code[(int)kFive[rnd(10)]], 5);
                    s.ones((8u - (s.n & 7u)) & 7u);
                    if (count == 0 && (rep & 1) == 0) s.ones(8);  // (no symbol from one byte; odd reps: the empty literal)
                    Case c{s.b.data(), (uint32_t)s.b.size(), 0, 0, 0, 0, 0, 0, rep & 1};
                    place_in(c, rnd(16));
                    place_out(c, res);
                    c.cap = c.n * 8u / 5u + ((rep & 2) ? rnd(5) : 0u);
                    const Got g = run_case(c);
                    bool ok = same(g, oracle_at(s.b, c.cap, false), c, "a");
                    if (ok && (g.cnt != count || g.path != (c.n ? kStagedBound : kEmpty))) {
                        printf("a: count %u decoded %u on path %s\n", count, g.cnt, kPathName[g.path]);
                        ok = false;
                    }
                    const Plan p = store_plan(c.out_mis + c.o0, g.cnt);
                    const uint32_t pc[5] = {p.head, p.lead, p.groups, p.trail, p.tail};
                    for (int k = 0; k < 5; ++k) g_piece[k] += pc[k] != 0u;
                    a_bad += !ok;
                    cases += 1;
                }
        printf("a store plan: %ld cases, %ld mismatches; pieces taken: head %ld lead %ld groups %ld trail %ld tail %ld\n", cases, a_bad,
               g_piece[0], g_piece[1], g_piece[2], g_piece[3], g_piece[4]);
        bad += a_bad;
    }

    // b, c. input placement, twice
    std::vector<Bytes> pool;
    {
        long cases = 0, b_bad = 0, c_bad = 0, past = 0;
        auto one = [&](const Bytes& lit, uint32_t res) {
            Case c{lit.data(), (uint32_t)lit.size(), 0, 0, 0, 0, 0, 0, 1};
            place_in(c, res);
            place_out(c, rnd(16));
            c.cap = c.n * 8u / 5u;
            const Ref& r = oracle_at(lit, c.cap, false);
            const Got g1 = run_case(c);
            b_bad += !same(g1, r, c, "b");
            c.fill = 0;
            const Got g2 = run_case(c);
            c_bad += !(same(g2, r, c, "c") && g1.cnt == g2.cnt && g1.st == g2.st && g1.bytes == g2.bytes);
            if (g1.path != kStagedBound) {
                printf("b: %u bytes not on the staged bound path\n", c.n);
                b_bad += 1;
            }
            // the walk's highest read is dword (X >> 5) + 2 with X <= the literal's end bit + 31
            const uint32_t sb = 32u + ((c.in_mis + c.p0) & 15u) * 8u;
            past += ((sb + c.n * 8u + 31u) >> 5) + 2u > 4u * kPersistSlotChunks;
            cases += 1;
        };
        for (uint32_t res = 0; res < 16; ++res)
            for (uint32_t L = 1; L <= kPersistSlotMax; ++L)
                for (int kind = 0; kind < kKinds; ++kind) {
                    pool.push_back(make_literal(kind, L));
                    one(pool.back(), res);
                }
        long nvec = 0;
        for (const Bytes& v : vectors)
            if (!v.empty() && v.size() <= kPersistSlotMax) {
                pool.push_back(v);
                nvec += 1;
                for (uint32_t res = 0; res < 16; ++res) one(v, res);
            }
        printf("b input placement: %ld cases (%ld error vectors), %ld mismatches\n", cases, nvec, b_bad);
        printf("c independence: %ld pairs, %ld mismatches, %ld may read past the slot's %u dwords\n", cases, c_bad, past,
               kPersistInStride);
        bad += b_bad + c_bad;
    }

    // d. short regions
    {
        long lits = 0, cases = 0, d_bad = 0, err_wins = 0, ovf_wins = 0;
        for (size_t i = 0; i < pool.size(); i += 6) {
            const Bytes& lit = pool[i];
            const uint32_t bound = (uint32_t)lit.size() * 8u / 5u;
            if (bound == 0u) continue;
            const Ref full = oracle_at(lit, bound, false);
            lits += 1;
            for (uint32_t cap = 0; cap < bound; ++cap) {
                Case c{lit.data(), (uint32_t)lit.size(), 0, 0, 0, 0, 0, cap, (int)(cap & 1u)};
                place_in(c, rnd(16));
                place_out(c, rnd(16));
                const Ref& r = oracle_at(lit, cap, false);
                const Got g = run_case(c);
                bool ok = same(g, r, c, "d");
                if (g.path != kStagedBytes) ok = false;
                if (r.st == 4 && g.cnt != cap) ok = false;  // (out_len = cap on overflow)
                if (full.st != 0 && full.st != 4) {  // an error behind the capacity: the overflow wins; at it: the error
                    ovf_wins += full.bytes.size() > cap && r.st == 4;
                    err_wins += full.bytes.size() == cap && r.st == full.st;
                }
                d_bad += !ok;
                cases += 1;
            }
        }
        printf("d short regions: %ld literals, %ld cases, %ld mismatches; error behind the capacity %ld, at it %ld\n", lits, cases,
               d_bad, ovf_wins, err_wins);
        bad += d_bad;
    }

    // e. the global walker
    {
        long cases = 0, e_bad = 0, guard2 = 0;
        auto one = [&](const Bytes& lit, uint32_t ores, uint32_t ires) {
            const uint32_t bound = (uint32_t)lit.size() * 8u / 5u;
            const uint32_t count = (uint32_t)oracle_at(lit, bound, true).bytes.size();
            uint32_t caps[5] = {bound, count, 0u, 0u, 0u};
            int nc = 2;
            if (count >= 1u) caps[nc++] = count - 1u;
            if (count >= 2u) caps[nc++] = count - 2u;
            caps[nc++] = 0u;
            for (int k = 0; k < nc; ++k) {
                Case c{lit.data(), (uint32_t)lit.size(), 0, 0, 0, 0, 0, caps[k], k & 1};
                place_in(c, ires);
                place_out(c, ores + 8u * rnd(2));  // (ores is a residue mod 8)
                const Got g = run_case(c);
                bool ok = same(g, oracle_at(lit, caps[k], true), c, "e");
                if (g.path != kGlobal) ok = false;
                guard2 += caps[k] + 1u == count || caps[k] + 2u == count;
                e_bad += !ok;
                cases += 1;
            }
        };
        for (uint32_t L = kPersistSlotMax + 1u; L <= 300u; ++L) {
            Bytes lits[kKinds];
            for (int kind = 0; kind < kKinds; ++kind) lits[kind] = make_literal(kind, L);
            for (uint32_t ores = 0; ores < 8; ++ores)
                for (uint32_t ires = 0; ires < 16; ++ires) one(lits[(L + ores + ires) % kKinds], ores, ires);
        }
        const uint32_t big[3] = {1024u, 2049u, 4095u};
        const int big_kinds[4] = {kKText, kKFive, kKLongLast, kKEos};
        for (uint32_t L : big)
            for (uint32_t i = 0; i < 16; ++i) one(make_literal(big_kinds[i % 4], L), i % 8, i);
        printf("e global walker: %ld cases, %ld mismatches, %ld at capacity count - 1 or count - 2\n", cases, e_bad, guard2);
        bad += e_bad;
    }

    // f. the dispatch
    {
        long cases = 0, f_bad = 0;
        for (uint32_t b0 = 0; b0 < 4096u + 16u; ++b0) {
            for (uint32_t nb = 0; nb <= 113u; ++nb, ++cases) {
                const uint32_t nch = ((b0 + nb + 15u) >> 4) - (b0 >> 4);
                f_bad += !(staged(b0, nb) && nch <= 8u && 4u * nch + 1u <= kPersistInStride);
            }
            f_bad += staged(b0, 114u);
            cases += 1;
        }
        // the decoded bound of a staged literal, 3 bytes of alignment, a body step's garbage and the dummy byte
        f_bad += !(kPersistSlotMax * 8u / 5u + 3u + 4u + 1u <= kPersistOutDw * 4u);
        printf("f dispatch: %ld cases, %ld mismatches\n", cases, f_bad);
        bad += f_bad;
    }

    printf("paths:");
    for (int p = 0; p < kPaths; ++p) printf(" %s %ld", kPathName[p], g_paths[p]);
    printf("\n%s: %ld mismatches\n", bad ? "FAIL" : "ok", bad);
    free(g_islot);
    free(g_oslot);
    return bad != 0;
}
