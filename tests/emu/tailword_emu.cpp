// Host replay of the wave kernel's fill trim (hpk_wave.h: the saved tail word and the carried status) with the REAL functions
// of loona_amd/csrc (hpk_walk.h as it is; tests/emu/shim.h stands in for the HIP builtins), under table kind 4:
//   a. tails alone: every bit pattern of 0..16 bits (0..13 bits at every X % 32, 14..16 at four), random patterns
//      of 17..30 bits, all ones and all zeros, behind random window bits and followed by random bits:
//        * the tail made from the saved word (tail12_word where the lane holds its dwords, tail12_begin_saved
//          later, the lane's dwords overwritten in between) equals tail12_begin after lit12_load at the same
//          state, field by field, and decodes the same image and output position;
//        * the status carried out of tail12_end (a slow lane: reloaded, checked steps, then the status at its
//          stop) equals residual_status of the window at the stop against the literal's end, or the body's status
//          where the body set one (then no bits are left);
//   b. whole literals through the lane protocol as the kernel runs it now (body steps, the word saved where the
//      body ends, masked tails, a reload for the slow lanes only, carried status), exact-bound regions back to
//      back, against the oracle.
// Test infrastructure only (tests/test_tailword_emulation.py). Exit status 0 = no mismatch.
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
constexpr uint32_t kMin = body_min<kTab>(), kTailMax = kMin - 1u;
static_assert(lut_bits<kTab>() == 13 && kMin == 31, "the 13-bit instantiation");

static hpk_tables T;
static long g_cases = 0, g_slow = 0, g_bad = 0, g_exh = 0, g_rand = 0;

static uint64_t g_sm = 0x9E3779B97F4A7C15ull;
static inline uint64_t sm64() {  // splitmix64
    uint64_t z = (g_sm += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

constexpr uint32_t kO0 = 16, kDmy = 48, kImgN = 64;

static void fail(const char* what, uint32_t rem, uint32_t pat, uint32_t al, uint32_t a, uint32_t b) {
    if (g_bad < 8) printf("tail word: rem %u pat %x al %u: %s (%u vs %u)\n", rem, pat, al, what, a, b);
    ++g_bad;
}

// One tail: `rem` bits `pat` (right-aligned) at bit 32 + al of a random window; st0: a status from the body
// (then rem is 0).
static void one_tail(uint32_t rem, uint32_t pat, uint32_t al, uint32_t st0 = HPK_OK) {
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
    Lit12 Z;
    Z.act = true;
    Z.idx = 0;
    Z.X = P + 31u;
    Z.Eb = Z.X + rem;
    Z.o = Z.o0 = kO0;
    Z.oend = kO0 + rem / 5;
    Z.st = st0;
    Z.prog = false;
    Z.more = false;
    lit12_load(Z, w32);
    const uint32_t Eb0 = Z.Eb;
    uint8_t ia[kImgN], ib[kImgN];
    memset(ia, 0xEE, sizeof ia);
    memset(ib, 0xEE, sizeof ib);
    // A: tail12_begin after lit12_load, the first slot's status from the window at the stop (v38..v41)
    Lit12 A = Z;
    lit12_load(A, w32);
    A.more = A.Eb - A.X >= 5u;
    Tail12 TA;
    tail12_begin(TA, A);
    // B: the word saved while the lane holds its dwords, which are then lost (the second literal's take their place)
    Lit12 B = Z;
    const uint32_t word = tail12_word(B);
    B.d0 = 0xDEADBEEFu, B.d1 = 0x0BADF00Du, B.d2 = 0xFEEDFACEu;
    B.more = B.Eb - B.X >= 5u;
    Tail12 TB;
    tail12_begin_saved(TB, word, B.Eb - B.X, B.o);
    if (TA.n != TB.n) fail("the saved word is not tail12_begin's", rem, pat, al, TB.n, TA.n);
    if (TA.rem != TB.rem || TA.used != TB.used || TA.o != TB.o) fail("the saved tail's other fields", rem, pat, al, TB.rem, TA.rem);
    for (int s = 0; s < 4; ++s) {
        tail12_look<kPred, kTab>(TA, lut, ia, kDmy);
        tail12_look<kPred, kTab>(TB, lut, ib, kDmy);
    }
    A.more &= tail12_end<kTab>(TA, A);
    const bool slow = tail12_end<kTab>(TB, B);
    B.more &= slow;
    if (slow) lit12_load(B, w32);  // the slow lanes alone take their dwords
    for (int g = 0; A.more && g < 64; ++g) lit12_step<kPred, true, kTab, true>(A, w32, lut, T.lo, ia, kDmy);
    for (int g = 0; B.more && g < 64; ++g) lit12_step<kPred, true, kTab, true>(B, w32, lut, T.lo, ib, kDmy);
    if (slow && B.st == HPK_OK) B.st = residual_status(B.Eb - B.X, win_at(w32, B.X - 31u));
    const uint32_t stB = B.st;  // carried
    const uint32_t stA = A.st != HPK_OK ? A.st : residual_status(Eb0 - A.X, win_at(w32, A.X - 31u));
    if (stA != stB) fail("the carried status", rem, pat, al, stB, stA);
    if (st0 != HPK_OK && stB != st0) fail("the body's status is not kept", rem, pat, al, stB, st0);
    if (A.o != B.o || A.X != B.X) fail("the stop", rem, pat, al, B.o, A.o);
    ia[kDmy] = ib[kDmy] = 0xEE;
    ia[kDmy + 1] = ib[kDmy + 1] = 0xEE;
    if (memcmp(ia, ib, kImgN) != 0) fail("the image", rem, pat, al, 0, 0);
    for (uint32_t j = 0; j < kImgN; ++j)
        if ((j < kO0 || j >= kO0 + rem / 5) && ib[j] != 0xEE) {
            fail("a byte outside the region", rem, pat, al, j, 0);
            break;
        }
    ++g_cases;
    g_slow += slow;
}

static void tails_alone(long nrand) {
    for (uint32_t rem = 0; rem <= 16; ++rem)
        for (uint32_t pat = 0; pat < (1u << rem); ++pat) {
            ++g_exh;
            if (rem <= 13)
                for (uint32_t al = 0; al < 32; ++al) one_tail(rem, pat, al);
            else
                for (uint32_t j = 0; j < 4; ++j) one_tail(rem, pat, (pat * 5u + 8u * j + rem) & 31u);
        }
    for (uint32_t rem = 17; rem <= kTailMax; ++rem) {
        for (long i = 0; i < nrand; ++i, ++g_rand) one_tail(rem, (uint32_t)sm64() & ((1u << rem) - 1u), (uint32_t)(i & 31));
        for (uint32_t al = 0; al < 32; ++al) {
            one_tail(rem, (1u << rem) - 1u, al);
            one_tail(rem, 0u, al);
        }
    }
    for (uint32_t al = 0; al < 32; ++al) {  // a status from the body: no bits left, the status stays
        one_tail(0, 0, al, HPK_EOS_IN_STRING);
        one_tail(0, 0, al, HPK_PADDING_TOO_LARGE);
    }
}

// ---- whole literals: tail_emu.cpp's mix through the lane protocol of the trimmed fill
typedef std::vector<std::vector<uint8_t>> Lits;

static void mixed_lits(Lits& lits, std::mt19937_64& rng, int nlit, int maxlen) {
    const char* text = "abcdefghijklmnopqrstuvwxyz0123456789-_=;,/.:ABC ";
    const char* five = "012aceiost";
    for (int i = 0; i < nlit; ++i) {
        int kind = rng() % 8, n = rng() % (maxlen + 1);
        std::vector<uint8_t> s(n);
        for (auto& c : s) c = kind == 0 ? five[rng() % 10] : kind == 1 ? text[rng() % strlen(text)] : (uint8_t)rng();
        std::vector<uint8_t> enc = s;  // (kinds 3..5: random bytes: padding errors, EOS, long codes)
        if (kind <= 2 || kind >= 6) {
            enc.assign(4 * s.size() + 8, 0);
            size_t el = 0;
            oracle_encode(s.data(), s.size(), enc.data(), enc.size(), &el);
            enc.resize(el);
        }
        if (kind == 4 && enc.size() > 2) enc[enc.size() - 1] &= 0xF0;
        if (kind == 5 && enc.size() > 4) {
            size_t p = rng() % (enc.size() - 3);
            enc[p] = enc[p + 1] = enc[p + 2] = enc[p + 3] = 0xFF;
        }
        if (kind == 7) enc.push_back(0xFF);  // too much padding
        lits.push_back(enc);
    }
}

static long run_lanes(const Lits& lits, std::mt19937_64& rng, long* slow_lanes, long* body_status) {
    long bad = 0;
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
        const uint32_t dmy = op + 64 + 4;
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
                    Z.o = Z.o0 = o0[u];
                    Z.st = HPK_OK;
                    Z.prog = false;
                    lit12_load(Z, w32);
                };
                Lit12 L, N;
                load(L, t1);
                bool body = L.Eb - L.X >= kMin;
                while (body) lit12_body<kPred, kTab>(L, w32, lut, T.lo, img.data(), body);
                // the first literal waits as (aX, aO, aSt, aAct) and its tail word
                const uint32_t aX = L.X, aO = L.o, aSt = L.st, aN = tail12_word(L);
                const bool aAct = L.act;
                if (pass == 0) *body_status += aSt != HPK_OK;
                load(L, t2);
                body = L.Eb - L.X >= kMin;
                while (body) lit12_body<kPred, kTab>(L, w32, lut, T.lo, img.data(), body);
                N = L;
                const uint32_t u1 = std::min<uint32_t>(t1, k - 1);
                L.X = aX, L.o = aO, L.st = aSt, L.act = aAct;  // (d0, d1, d2 stay the second literal's)
                L.Eb = p0[u1] * 8u + 31u + (aAct ? nb[u1] * 8u : 0u);
                L.o0 = o0[u1];
                if (aSt != HPK_OK) L.Eb = L.X;
                L.more = L.Eb - L.X >= 5u;
                N.more = N.Eb - N.X >= 5u;
                Tail12 TL, TN;
                tail12_begin_saved(TL, aN, L.Eb - L.X, L.o);
                tail12_begin(TN, N);
                for (int s = 0; s < 4; ++s) {
                    tail12_look<kPred, kTab>(TL, lut, img.data(), dmy);
                    tail12_look<kPred, kTab>(TN, lut, img.data(), dmy);
                }
                const bool slowL = tail12_end<kTab>(TL, L);
                L.more &= slowL;
                N.more &= tail12_end<kTab>(TN, N);
                if (pass == 0) *slow_lanes += (int)slowL;
                if (slowL) lit12_load(L, w32);
                for (int guard = 0; (L.more || N.more) && guard < 1000000; ++guard) {
                    if (L.more) lit12_step<kPred, true, kTab, true>(L, w32, lut, T.lo, img.data(), dmy);
                    if (N.more) lit12_step<kPred, true, kTab, true>(N, w32, lut, T.lo, img.data(), dmy);
                }
                if (slowL && L.st == HPK_OK) L.st = residual_status(L.Eb - L.X, win_at(w32, L.X - 31u));
                if (L.act) olen[t1] = L.o - L.o0, ost[t1] = L.st;  // carried: no window read here
                if (N.act) olen[t2] = N.o - N.o0, ost[t2] = lit12_status(N);
            }
            if (pass == 0) {
                olen0 = olen, ost0 = ost, img0 = img;
            } else if (olen != olen0 || ost != ost0 || img != img0) {
                if (bad < 5) printf("lanes: the fill at %zu depends on the dword before its window\n", f);
                ++bad;
            }
        }
        for (size_t t = 0; t < k; ++t) {
            std::vector<uint8_t> ref(cap[t] + 8);
            size_t rl = 0;
            const int rs = oracle_decode(lits[f + t].data(), nb[t], ref.data(), ref.size(), &rl);
            const bool ok = rs == (int)ost[t] && rl == olen[t] && memcmp(ref.data(), img.data() + o0[t], rl) == 0;
            if (!ok && bad < 5)
                printf("lanes: literal %zu (%u B): status %u vs %d, length %u vs %zu\n", f + t, nb[t], ost[t], rs, olen[t], rl);
            bad += !ok;
        }
        bool guard_ok = true;
        for (uint32_t j = 0; j < ofirst; ++j) guard_ok &= img[j] == 0xEE;
        for (uint32_t j = op; j < op + 64; ++j) guard_ok &= img[j] == 0xEE;
        if (!guard_ok) {
            if (bad < 5) printf("lanes: a byte outside the regions written\n");
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
    const long nrand = argc > 2 ? atol(argv[2]) : 80000;  // random patterns per length 17..30
    g_sm += (uint64_t)seed * 0x2545F4914F6CDD1Dull;
    tails_alone(nrand);
    printf("tails alone: %ld cases (%ld patterns of 0..16 bits, %ld random), %ld slow, %ld mismatches\n", g_cases, g_exh, g_rand,
           g_slow, g_bad);
    std::mt19937_64 rng(seed);
    Lits mix;
    mixed_lits(mix, rng, 12000, 70);
    mixed_lits(mix, rng, 2000, 400);
    long slow_lanes = 0, body_status = 0;
    const long lanes_bad = run_lanes(mix, rng, &slow_lanes, &body_status);
    printf("whole literals: %zu literals, %ld slow first tails, %ld body statuses, %ld mismatches\n", mix.size(), slow_lanes,
           body_status, lanes_bad);
    const long bad = g_bad + lanes_bad;
    printf("%s: %ld mismatches\n", bad ? "FAIL" : "ok", bad);
    return bad != 0;
}
