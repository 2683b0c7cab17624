// Host emulation of the lane walk on the 13-bit two-symbol table (kTab 4, decode v39) with the REAL functions
// of loona_amd/csrc (hpk_walk.h as it is; tests/emu/shim.h stands in for the HIP builtins):
//   a. tails alone, lit12_tail<.., 4> with its checked fallback against the checked tail loop
//      (lit12_step<.., 4, kMore>) from the same state: every bit pattern of 0..18 bits (0..13 bits at every
//      X % 32, 14..18 at four), random patterns of 19..30 bits, all ones, all zeros, and every code of >= 13
//      bits (EOS too) at every offset of a tail that shorter codes can reach, followed by ones, at every
//      X % 32: image, final o and status identical, nothing but the exact-bound region and the dummy slot
//      written;
//   b. valid tails (codes of <= 13 bits, then 0..7 ones: every sequence of code lengths, and random symbol
//      sequences) never take the fallback;
//   c. whole literals against the oracle, through the wave kernel's lane protocol (lit12_body<.., 4> while
//      >= body_min<4>() = 31 bits are left, the masked tails, the checked steps for the slow lanes) and
//      through the checked step alone, in exact-bound regions back to back: literals whose codes take
//      exactly 24..48 bits (the body-min boundary at 29..32), literals made only of the 13-bit pairs 6+7,
//      7+6, 5+8, 8+5, only of the six 13-bit codes, mixes of the two, and tail_emu.cpp's mix (random text,
//      random bytes, EOS, bad and long padding).
// Test infrastructure only (tests/test_walk13_emulation.py). Exit status 0 = no mismatch and no slow valid tail.
#include "shim.h"
#include "hpk_walk.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
extern "C" int oracle_decode(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len);
extern "C" int oracle_encode(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len);
using namespace hpkdec;

constexpr int kTab = 4;
constexpr uint32_t kBits = lut_bits<kTab>(), kMin = body_min<kTab>(), kTailMax = kMin - 1u;
static_assert(kBits == 13 && kMin == 31, "the 13-bit instantiation");

static hpk_tables T;
static long g_cases = 0, g_slow = 0, g_bad = 0;

static uint64_t g_sm = 0x9E3779B97F4A7C15ull;
static inline uint64_t sm64() {  // splitmix64
    uint64_t z = (g_sm += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

constexpr uint32_t kO0 = 16, kDmy = 48, kImgN = 64;

// One tail: `rem` bits `pat` (right-aligned) at bit 32 + al of a random window, a body status `st0`
// (then rem is 0). Returns whether the masked tail left the lane as slow.
static bool one_tail(uint32_t rem, uint32_t pat, uint32_t al, uint32_t st0 = HPK_OK) {
    uint32_t w32[8];
    for (int j = 0; j < 8; j += 2) {
        const uint64_t r = sm64();
        w32[j] = (uint32_t)r;
        w32[j + 1] = (uint32_t)(r >> 32);
    }
    const uint32_t P = 32 + al;
    for (uint32_t b = 0; b < rem; ++b) {
        const uint32_t p = P + b, bit = (pat >> (rem - 1 - b)) & 1u;
        w32[p >> 5] = (w32[p >> 5] & ~(1u << (31 - (p & 31)))) | (bit << (31 - (p & 31)));
    }
    const uint32_t* lut = T.lut13;
    const uint32_t cap = rem / 5;  // the exact bound: a code is >= 5 bits
    Lit12 Z;
    Z.act = true;
    Z.idx = 0;
    Z.X = P + 31u;
    Z.Eb = Z.X + rem;
    Z.o = Z.o0 = kO0;
    Z.oend = kO0 + cap;
    Z.st = st0;
    Z.prog = false;
    Z.more = false;
    lit12_load(Z, w32);
    uint8_t ia[kImgN], ib[kImgN];
    memset(ia, 0xEE, sizeof ia);
    memset(ib, 0xEE, sizeof ib);
    Lit12 A = Z;  // the checked tail loop
    A.more = A.Eb - A.X >= 5u;
    for (int g = 0; A.more && g < 64; ++g) lit12_step<kPred, true, kTab, true>(A, w32, lut, T.lo, ia, kDmy);
    Lit12 B = Z;  // the masked tail, then the checked steps if it says slow
    const bool slow = lit12_tail<kPred, kTab>(B, lut, ib, kDmy);
    if (slow) {
        const bool same = B.X == Z.X && B.o == Z.o && B.st == Z.st && B.Eb == Z.Eb && B.d0 == Z.d0 && B.d1 == Z.d1 && B.d2 == Z.d2;
        if (!same) {
            if (g_bad < 8) printf("tail: rem %u pat %x al %u: a slow lane's state changed\n", rem, pat, al);
            ++g_bad;
        }
        B.more = B.Eb - B.X >= 5u;
        for (int g = 0; B.more && g < 64; ++g) lit12_step<kPred, true, kTab, true>(B, w32, lut, T.lo, ib, kDmy);
    }
    ia[kDmy] = ib[kDmy] = 0xEE;  // the dummy slot: anything
    bool ok = A.o == B.o && lit12_status(A) == lit12_status(B) && memcmp(ia, ib, kImgN) == 0 && A.o - kO0 <= cap;
    for (uint32_t j = 0; j < kImgN; ++j)
        if ((j < kO0 || j >= kO0 + cap) && (ia[j] != 0xEE || ib[j] != 0xEE)) ok = false;
    if (!ok) {
        if (g_bad < 8)
            printf("tail: rem %u pat %x al %u st0 %u: o %u vs %u, status %u vs %u (slow %d)\n", rem, pat, al, st0, B.o, A.o,
                   lit12_status(B), lit12_status(A), (int)slow);
        ++g_bad;
    }
    ++g_cases;
    g_slow += slow;
    return slow;
}

static long g_exh = 0, g_rand = 0, g_long = 0;

static void tails_alone(long nrand) {
    for (uint32_t rem = 0; rem <= 18; ++rem)
        for (uint32_t pat = 0; pat < (1u << rem); ++pat) {
            ++g_exh;
            if (rem <= 13)
                for (uint32_t al = 0; al < 32; ++al) one_tail(rem, pat, al);
            else
                for (uint32_t j = 0; j < 4; ++j) one_tail(rem, pat, (pat * 5u + 8u * j + rem) & 31u);
        }
    for (uint32_t rem = 19; rem <= kTailMax; ++rem) {
        for (long i = 0; i < nrand; ++i, ++g_rand) one_tail(rem, (uint32_t)sm64() & ((1u << rem) - 1u), (uint32_t)(i & 31));
        for (uint32_t al = 0; al < 32; ++al) {
            one_tail(rem, (1u << rem) - 1u, al);
            one_tail(rem, 0u, al);
        }
    }
    // every code of >= 13 bits (EOS included) at every offset that codes of <= 12 bits can make up, then ones
    std::vector<int> by_len[13];
    for (int s = 0; s < 256; ++s)
        if (T.len[s] <= 12) by_len[T.len[s]].push_back(s);
    for (int s = 0; s < HPK_NSYM; ++s) {
        const uint32_t len = T.len[s];
        if (len < 13) continue;
        for (uint32_t off = 0; off + len <= kTailMax; ++off) {
            // a prefix of exactly `off` bits: greedy over the code lengths, retried at random
            uint32_t pre = 0, got = 0;
            bool made = off == 0;
            for (int tries = 0; !made && tries < 64; ++tries) {
                pre = 0;
                got = 0;
                while (got < off) {
                    const uint32_t l = 5 + sm64() % 8;
                    if (by_len[l].empty() || got + l > off) {
                        if (off - got < 5) break;
                        continue;
                    }
                    pre = (pre << l) | T.code[by_len[l][sm64() % by_len[l].size()]];
                    got += l;
                }
                made = got == off;
            }
            if (!made) continue;  // (1..4 and 9 bits: no sequence of codes)
            for (uint32_t rem = off + len; rem <= kTailMax; ++rem) {
                const uint32_t pad = rem - off - len;
                const uint32_t pat = (uint32_t)(((((uint64_t)pre << len) | T.code[s]) << pad) | ((1u << pad) - 1u));
                for (uint32_t al = 0; al < 32; ++al) one_tail(rem, pat, al), ++g_long;
            }
        }
    }
    // a status from the body: no bits left, the status stays
    for (uint32_t al = 0; al < 32; ++al) {
        one_tail(0, 0, al, HPK_EOS_IN_STRING);
        one_tail(0, 0, al, HPK_PADDING_TOO_LARGE);
    }
}

// Valid tails: codes of <= 13 bits, then 0..7 ones; none may be slow.
static long valid_tails(long nrand) {
    std::vector<int> by_len[14];
    std::vector<int> shorts;
    for (int s = 0; s < 256; ++s)
        if (T.len[s] <= kBits) by_len[T.len[s]].push_back(s), shorts.push_back(s);
    long slow = 0, n = 0;
    struct Fr { uint32_t bits, pat; int next; };
    std::vector<Fr> stack{{0u, 0u, 5}};
    while (!stack.empty()) {  // depth-first over the length sequences
        Fr& f = stack.back();
        if (f.next == 5)  // this prefix itself, with every padding
            for (uint32_t pad = 0; pad <= 7 && f.bits + pad <= kTailMax; ++pad)
                for (uint32_t al = 0; al < 32; ++al)
                    slow += one_tail(f.bits + pad, (f.pat << pad) | ((1u << pad) - 1u), al), ++n;
        int l = f.next;
        while (l <= (int)kBits && (by_len[l].empty() || f.bits + l > kTailMax)) ++l;
        if (l > (int)kBits) {
            stack.pop_back();
            continue;
        }
        f.next = l + 1;
        const int s = by_len[l][sm64() % by_len[l].size()];
        const Fr child{f.bits + (uint32_t)l, (f.pat << l) | T.code[s], 5};  // (f may move: made before the push)
        stack.push_back(child);
    }
    for (long i = 0; i < nrand; ++i) {
        const uint32_t pad = sm64() % 8;
        uint32_t bits = 0, pat = 0;
        for (int c = 0; c < 6; ++c) {
            const std::vector<int>& pool = (i & 1) ? shorts : by_len[5 + sm64() % 4];
            const int sy = pool[sm64() % pool.size()];
            if (bits + T.len[sy] + pad > kTailMax) break;
            pat = (pat << T.len[sy]) | T.code[sy];
            bits += T.len[sy];
            if (sm64() % 8 == 0) break;
        }
        slow += one_tail(bits + pad, (pat << pad) | ((1u << pad) - 1u), (uint32_t)(i & 31)), ++n;
    }
    printf("valid tails: %ld cases, %ld slow\n", n, slow);
    return slow;
}

// ---- whole literals
typedef std::vector<std::vector<uint8_t>> Lits;

static std::vector<uint8_t> encode(const std::vector<uint8_t>& s) {
    std::vector<uint8_t> enc(4 * s.size() + 8);
    size_t el = 0;
    oracle_encode(s.data(), s.size(), enc.data(), enc.size(), &el);
    enc.resize(el);
    return enc;
}

// strings whose codes take exactly `bits` bits (then the encoder's padding)
static void sweep_lits(Lits& out, std::mt19937_64& rng, int per_len) {
    std::vector<int> by_len[31];
    for (int s = 0; s < 256; ++s) by_len[T.len[s]].push_back(s);
    for (uint32_t bits = 24; bits <= 48; ++bits)
        for (int i = 0; i < per_len; ++i) {
            for (;;) {
                std::vector<uint8_t> s;
                uint32_t got = 0;
                while (got < bits) {
                    // mostly 5..8-bit codes; now and then any length up to 30
                    const uint32_t l = rng() % 16 ? 5 + rng() % 4 : 5 + rng() % 26;
                    if (by_len[l].empty() || got + l > bits) {
                        if (bits - got < 5) break;
                        continue;
                    }
                    s.push_back((uint8_t)by_len[l][rng() % by_len[l].size()]);
                    got += l;
                }
                if (got != bits) continue;
                out.push_back(encode(s));
                break;
            }
        }
}

// literals made only of the 13-bit pairs, only of the six 13-bit codes, and of both
static void pair_lits(Lits& out, std::mt19937_64& rng, int n) {
    std::vector<int> by_len[31], thirteen;
    for (int s = 0; s < 256; ++s) by_len[T.len[s]].push_back(s);
    thirteen = by_len[13];  // symbols 0, '$', '@', '[', ']', '~'
    static const int pl[4][2] = {{6, 7}, {7, 6}, {5, 8}, {8, 5}};
    for (int i = 0; i < n; ++i) {
        const int kind = i % 3, units = 1 + (int)(rng() % 40);
        std::vector<uint8_t> s;
        for (int u = 0; u < units; ++u) {
            if (kind == 0 || (kind == 2 && rng() % 2)) {
                const int* p = pl[rng() % 4];
                s.push_back((uint8_t)by_len[p[0]][rng() % by_len[p[0]].size()]);
                s.push_back((uint8_t)by_len[p[1]][rng() % by_len[p[1]].size()]);
            } else {
                s.push_back((uint8_t)thirteen[rng() % thirteen.size()]);
            }
        }
        out.push_back(encode(s));
    }
}

static void mixed_lits(Lits& lits, std::mt19937_64& rng, int nlit, int maxlen) {
    const char* text = "abcdefghijklmnopqrstuvwxyz0123456789-_=;,/.:ABC ";
    const char* five = "012aceiost";
    for (int i = 0; i < nlit; ++i) {
        int kind = rng() % 8, n = rng() % (maxlen + 1);
        std::vector<uint8_t> s(n);
        for (auto& c : s) c = kind == 0 ? five[rng() % 10] : kind == 1 ? text[rng() % strlen(text)] : (uint8_t)rng();
        std::vector<uint8_t> enc = (kind <= 2 || kind >= 6) ? encode(s) : s;  // (else random bytes: padding errors, EOS, long codes)
        if (kind == 4 && enc.size() > 2) enc[enc.size() - 1] &= 0xF0;
        if (kind == 5 && enc.size() > 4) {
            size_t p = rng() % (enc.size() - 3);
            enc[p] = enc[p + 1] = enc[p + 2] = enc[p + 3] = 0xFF;
        }
        if (kind == 7) enc.push_back(0xFF);  // too much padding
        lits.push_back(enc);
    }
}

// checked: the checked step alone; else the wave kernel's lane protocol
static int run_lanes(const Lits& lits, std::mt19937_64& rng, bool checked, long* slow_lanes, const char* what) {
    int bad = 0;
    for (size_t f = 0; f < lits.size(); f += 128) {
        const size_t k = std::min<size_t>(128, lits.size() - f);
        const uint32_t mis = rng() % 16;  // (0: a literal at byte 0 of the window, the guard dword in front of it)
        std::vector<uint8_t> win(mis);
        std::vector<uint32_t> p0(k), nb(k), o0(k), cap(k);
        const uint32_t ofirst = 4 + rng() % 4;
        uint32_t op = ofirst;
        for (size_t t = 0; t < k; ++t) {
            p0[t] = win.size();
            nb[t] = lits[f + t].size();
            win.insert(win.end(), lits[f + t].begin(), lits[f + t].end());
            o0[t] = op;
            cap[t] = nb[t] * 8 / 5;
            op += cap[t];
        }
        // The window as the walk may read it and not a dword more, so that a host sanitizer sees the true edges: one guard
        // dword in front (lit12_load reads the dword before the one holding X: w32[-1] for a literal at byte 0 of the
        // window, which mis == 0 places there), the literals, and the two dwords a step reads ahead of the one holding X
        // ((X >> 5) + 1 and + 2, X <= Eb). Bytes past the last literal are 0x5A.
        const size_t nd = (win.size() * 8 + 31) / 32 + 3;
        win.resize(nd * 4, 0x5A);
        std::vector<uint32_t> store(1 + nd, 0);
        uint32_t* const w32 = store.data() + 1;
        for (size_t j = 0; j < nd; ++j)
            w32[j] = ((uint32_t)win[4 * j] << 24) | ((uint32_t)win[4 * j + 1] << 16) | ((uint32_t)win[4 * j + 2] << 8) | win[4 * j + 3];
        std::vector<uint8_t> img(op + 256 + 64, 0xEE);
        const uint32_t dmy = op + 64 + 4;  // the lane's dummy dword, past the regions
        std::vector<uint32_t> olen(k), ost(k);
        const uint32_t* lut = T.lut13;
        // The guard dword's value must not reach a result (lit12_load's contract, hpk_walk.h): the fill runs twice, with it
        // all zeros and all ones, and must give the same lengths, statuses and image, byte for byte.
        std::vector<uint32_t> olen0, ost0;
        std::vector<uint8_t> img0;
        for (int pass = 0; pass < 2; ++pass) {
            store[0] = pass ? 0xFFFFFFFFu : 0x00000000u;
            img.assign(img.size(), 0xEE);
            olen.assign(k, 0);
            ost.assign(k, 0);
            for (int lane = 63; lane >= 0; --lane) {
                const uint32_t t1 = lane, t2 = 127 - lane;
                auto load = [&](Lit12& Z, uint32_t tt) {
                    const uint32_t u = std::min<uint32_t>(tt, k - 1);
                    Z.act = tt < k;
                    Z.idx = tt;
                    Z.X = p0[u] * 8u + 31u;
                    Z.Eb = Z.X + (Z.act ? nb[u] * 8u : 0u);
                    Z.o = o0[u];
                    Z.o0 = o0[u];
                    Z.st = HPK_OK;
                    Z.prog = false;
                    lit12_load(Z, w32);
                };
                Lit12 L, N;
                load(L, t1);
                load(N, t2);
                const uint32_t u1 = std::min<uint32_t>(t1, k - 1);
                if (!checked) {
                    bool body = L.Eb - L.X >= kMin;
                    while (body) lit12_body<kPred, kTab>(L, w32, lut, T.lo, img.data(), body);
                    Lit12 A = L;
                    L = N;
                    body = L.Eb - L.X >= kMin;
                    while (body) lit12_body<kPred, kTab>(L, w32, lut, T.lo, img.data(), body);
                    N = L;
                    L = A;  // restored as the kernel does: Eb from the queue entry, window reloaded at X
                    L.Eb = L.st != HPK_OK ? L.X : p0[u1] * 8u + 31u + (L.act ? nb[u1] * 8u : 0u);
                    lit12_load(L, w32);
                }
                L.more = L.Eb - L.X >= 5u;
                N.more = N.Eb - N.X >= 5u;
                if (!checked) {  // hpk_wave.h's tail block: the two chains' lookups in turn
                    Tail12 TL, TN;
                    tail12_begin(TL, L);
                    tail12_begin(TN, N);
                    for (int s = 0; s < 4; ++s) {
                        tail12_look<kPred, kTab>(TL, lut, img.data(), dmy);
                        tail12_look<kPred, kTab>(TN, lut, img.data(), dmy);
                    }
                    L.more &= tail12_end<kTab>(TL, L);
                    N.more &= tail12_end<kTab>(TN, N);
                    if (pass == 0) *slow_lanes += (int)L.more + (int)N.more;
                }
                for (int guard = 0; (L.more || N.more) && guard < 1000000; ++guard) {
                    if (L.more) lit12_step<kPred, true, kTab, true>(L, w32, lut, T.lo, img.data(), dmy);
                    if (N.more) lit12_step<kPred, true, kTab, true>(N, w32, lut, T.lo, img.data(), dmy);
                }
                if (L.act) {
                    const uint32_t Eb = p0[u1] * 8u + 31u + nb[u1] * 8u;
                    olen[t1] = L.o - L.o0;
                    ost[t1] = L.st != HPK_OK ? L.st : residual_status(Eb - L.X, win_at(w32, L.X - 31u));
                }
                if (N.act) olen[t2] = N.o - N.o0, ost[t2] = lit12_status(N);
            }
            if (pass == 0) {
                olen0 = olen, ost0 = ost, img0 = img;
            } else if (olen != olen0 || ost != ost0 || img != img0) {
                if (bad < 5) printf("%s: the fill at %zu depends on the dword before its window\n", what, f);
                ++bad;
            }
        }
        for (size_t t = 0; t < k; ++t) {
            std::vector<uint8_t> ref(cap[t] + 8);
            size_t rl = 0;
            const int rs = oracle_decode(lits[f + t].data(), nb[t], ref.data(), ref.size(), &rl);
            const bool ok = rs == (int)ost[t] && rl == olen[t] && memcmp(ref.data(), img.data() + o0[t], rl) == 0;
            if (!ok && bad < 5)
                printf("%s%s: literal %zu (%u B): status %u vs %d, length %u vs %zu\n", what, checked ? " (checked)" : "", f + t,
                       nb[t], ost[t], rs, olen[t], rl);
            bad += !ok;
        }
        bool guard_ok = true;
        for (uint32_t j = 0; j < ofirst; ++j) guard_ok &= img[j] == 0xEE;
        for (uint32_t j = op; j < op + 64; ++j) guard_ok &= img[j] == 0xEE;
        if (!guard_ok) {
            if (bad < 5) printf("%s: a byte outside the regions written\n", what);
            ++bad;
        }
    }
    return bad;
}

int main(int argc, char** argv) {
    if (hpk_build_tables(&T)) {
        printf("table build failed\n");
        return 1;
    }
    const int seed = argc > 1 ? atoi(argv[1]) : 1;
    const long nrand = argc > 2 ? atol(argv[2]) : 90000;  // random patterns per length 19..30
    g_sm += (uint64_t)seed * 0x2545F4914F6CDD1Dull;
    tails_alone(nrand);
    printf("tails alone: %ld cases (%ld patterns of 0..18 bits, %ld random, %ld long-code), %ld slow, %ld mismatches\n", g_cases,
           g_exh, g_rand, g_long, g_slow, g_bad);
    const long vslow = valid_tails(nrand);
    std::mt19937_64 rng(seed);
    long slow_lanes = 0, lanes_bad = 0, nl = 0;
    {
        Lits sweep, pairs, mix;
        sweep_lits(sweep, rng, 400);
        pair_lits(pairs, rng, 3000);
        mixed_lits(mix, rng, 4000, 70);
        mixed_lits(mix, rng, 1000, 400);
        for (int c = 0; c < 2; ++c) {
            lanes_bad += run_lanes(sweep, rng, c == 1, &slow_lanes, "sweep 24..48 bits");
            lanes_bad += run_lanes(pairs, rng, c == 1, &slow_lanes, "13-bit pairs and codes");
            lanes_bad += run_lanes(mix, rng, c == 1, &slow_lanes, "mix");
        }
        nl = (long)(sweep.size() + pairs.size() + mix.size());
        printf("whole literals: %ld literals (%zu swept, %zu of 13-bit pairs and codes), %ld slow tails, %ld mismatches\n", nl,
               sweep.size(), pairs.size(), slow_lanes, lanes_bad);
    }
    const long bad = g_bad + lanes_bad;
    printf("%s: %ld mismatches, %ld valid tails slow\n", bad || vslow ? "FAIL" : "ok", bad, vslow);
    return bad != 0 || vslow != 0;
}
