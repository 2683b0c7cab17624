// Host emulation of the lane loop's round of nested body steps (lit12_round, decode v41) with the REAL functions
// of loona_amd/csrc (hpk_walk.h as it is; tests/emu/shim.h stands in for the HIP builtins), one lane at a time
// (the round's wave-wide `any` is the lane's own flag). For every case the literal is walked twice from the same
// state: step by step with lit12_body (its leading-ones block inline), and round by round with
// lit12_round<.., 4 steps, kDefer> for kDefer 0, 1 and 2. After EVERY round the round walk's X, o, st, Eb, dword
// pair, `body` and whole image must be those of the step walk after some 1..4 of its steps (a parked lane loses
// step slots, never a step); when both bodies have ended the masked tail and the checked steps finish both, and
// a literal of whole bytes is compared with the oracle (bytes, length, status). Nothing but the literal's
// exact-bound region and the dummy slot may be written. Cases (13-bit table, body_min 31, <= 26 bits a step):
//   a. every remaining-bit count at a round's start from 0 to 31 + 4 * 26 + 13, so that the body ends after 0, 1,
//      2, 3 and 4 steps, codes of <= 13 bits and 0..7 bits of padding, at every X % 32;
//   b. every code longer than 13 bits, and EOS, as the first and as the second lookup of each of a round's four
//      steps (the lookups before it hold one 7-bit code each), followed by 0..4 more codes and padding (it
//      fits), or cut after 18.. bits by the literal's end (PaddingTooLarge; EOS whole: EOSInString);
//   c. two long codes in one round;
//   d. a step that ends the literal exactly (a short code and a long one of >= 31 bits together);
//   e. a mix of text, random bytes, runs of ones, bad and long padding.
// Test infrastructure only (tests/test_round_emulation.py). Exit status 0 = no mismatch.
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

constexpr int kTab = 4, kSteps = 4;
constexpr uint32_t kBits = lut_bits<kTab>(), kMin = body_min<kTab>();
static_assert(kBits == 13 && kMin == 31, "the 13-bit instantiation");
constexpr uint32_t kWinDw = 48, kMaxBits = (kWinDw - 6) * 32, kO0 = 16, kImgN = 512, kDmy = kImgN - 8;

static hpk_tables T;
static std::vector<int> by_len[31];
static std::mt19937_64 rng;
static long g_cases = 0, g_rounds = 0, g_bad = 0, g_oracle = 0;
static long g_first[kSteps + 1];     // (a) steps of the step walk in a literal's first round (kDefer 0)
static long g_place[kSteps][2];      // long codes handled in the body, by step of the round and lookup (kDefer 0)
static long g_two = 0, g_exact = 0;  // rounds with two long codes; steps that ended a literal exactly
static long g_ptl = 0, g_eos = 0;    // statuses set in the body
static long g_parked[kSteps];        // (kDefer 1, 2) steps of the step walk matched by a round that a lane left parked

struct Bits {
    std::vector<uint8_t> b;
    void put(uint32_t v, uint32_t n) {
        for (uint32_t i = 0; i < n; ++i) b.push_back((v >> (n - 1 - i)) & 1u);
    }
    void code(int s) { put(T.code[s], T.len[s]); }
    void ones(uint32_t n) {
        for (uint32_t i = 0; i < n; ++i) b.push_back(1);
    }
    void pad() { ones((8 - b.size() % 8) % 8); }
    int any(int l) { return by_len[l][rng() % by_len[l].size()]; }
};

struct Run {
    Lit12 L;
    bool body;
    uint8_t img[kImgN];
};

static bool same(const Run& a, const Run& b) {
    return a.L.X == b.L.X && a.L.o == b.L.o && a.L.st == b.L.st && a.L.Eb == b.L.Eb && a.L.d0 == b.L.d0 && a.L.d1 == b.L.d1 &&
           a.L.d2 == b.L.d2 && a.body == b.body && memcmp(a.img, b.img, kImgN) == 0;
}

// what the second lookup of a body step at L's position holds: 0 = no code (the step takes the leading-ones block)
static uint32_t peek_u2(const Lit12& L, bool& first) {
    const uint32_t w = __builtin_amdgcn_alignbit(L.d0, L.d1, ~L.X);
    const uint32_t e1 = T.lut13[w >> (32 - kBits)], u1 = HPK_L3_HELD(e1);
    first = u1 == 0u;
    return HPK_L3_HELD(T.lut13[(w << u1) >> (32 - kBits)]);
}

static void finish(Run& R, const uint32_t* w32) {  // the lane loop's tails
    R.L.more = R.L.Eb - R.L.X >= 5u;
    R.L.more &= lit12_tail<kPred, kTab>(R.L, T.lut13, R.img, kDmy);
    for (int g = 0; R.L.more && g < 4096; ++g) lit12_step<kPred, true, kTab, true>(R.L, w32, T.lut13, T.lo, R.img, kDmy);
}

template <int kDefer>
static bool round_walk(const Run& Z, const uint32_t* w32, Run& B, const char*& why) {
    Run A = Z;
    B = Z;
    bool first_round = true;
    for (int guard = 0; B.body; ++guard) {
        if (guard > 4096) return why = "the round walk does not end", false;
        lit12_round<kPred, kTab, kSteps, kDefer>(B.L, w32, T.lut13, T.lo, B.img, B.body, [](bool p) { return p; });
        int j = 0, longs = 0;
        bool match = false;
        while (!match && A.body && j < kSteps) {
            bool first;
            const bool lng = peek_u2(A.L, first) == 0u;
            lit12_body<kPred, kTab>(A.L, w32, T.lut13, T.lo, A.img, A.body);
            if (kDefer == 0 && lng) {
                ++g_place[j][first ? 0 : 1];
                ++longs;
                g_ptl += A.L.st == HPK_PADDING_TOO_LARGE;
                g_eos += A.L.st == HPK_EOS_IN_STRING;
            }
            if (kDefer == 0 && A.L.st == HPK_OK && A.L.X == A.L.Eb) ++g_exact;
            ++j;
            match = same(A, B);
            if (kDefer != 0 && lng && !match) return why = "a parked lane's state is not the step walk's behind its long code", false;
            if (kDefer != 0 && lng) ++g_parked[j - 1];
        }
        if (!match) return why = "a round's state is not the step walk's after 1..4 steps", false;
        if (kDefer == 0 && j != kSteps && A.body) return why = "an inline round stopped early", false;
        if (kDefer == 0) {
            g_two += longs >= 2;
            if (first_round) ++g_first[j];
            ++g_rounds;
        }
        first_round = false;
    }
    if (A.body) return why = "the step walk's body goes on", false;
    finish(A, w32);
    finish(B, w32);
    A.img[kDmy] = B.img[kDmy] = 0xEE;
    if (!(A.L.o == B.L.o && lit12_status(A.L) == lit12_status(B.L) && memcmp(A.img, B.img, kImgN) == 0))
        return why = "the finished walks differ", false;
    return true;
}

// One literal: its bits at bit 32 + al of a window of random bits.
static void one_case(const Bits& lit, uint32_t al, const char* what) {
    const uint32_t nb = (uint32_t)lit.b.size();
    if (nb > kMaxBits) return;
    uint32_t w32[kWinDw];
    for (uint32_t j = 0; j < kWinDw; ++j) w32[j] = (uint32_t)rng();
    const uint32_t P = 32 + al;
    for (uint32_t i = 0; i < nb; ++i) {
        const uint32_t p = P + i;
        w32[p >> 5] = (w32[p >> 5] & ~(1u << (31 - (p & 31)))) | ((uint32_t)lit.b[i] << (31 - (p & 31)));
    }
    const uint32_t cap = nb / 5;  // the exact bound: a code is >= 5 bits
    Run Z;
    memset(Z.img, 0xEE, sizeof Z.img);
    Z.L.act = true;
    Z.L.idx = 0;
    Z.L.X = P + 31u;
    Z.L.Eb = Z.L.X + nb;
    Z.L.o = Z.L.o0 = kO0;
    Z.L.oend = kO0 + cap;
    Z.L.st = HPK_OK;
    Z.L.prog = false;
    Z.L.more = false;
    lit12_load(Z.L, w32);
    Z.body = nb >= kMin;
    if (!Z.body) ++g_first[0];
    Run R[3];
    const char* why = "";
    bool ok = round_walk<0>(Z, w32, R[0], why);
    ok = ok && round_walk<1>(Z, w32, R[1], why);
    ok = ok && round_walk<2>(Z, w32, R[2], why);
    for (int d = 0; ok && d < 3; ++d)
        for (uint32_t j = 0; j < kImgN; ++j)
            if ((j < kO0 || j >= kO0 + cap) && j != kDmy && R[d].img[j] != 0xEE) ok = false, why = "a byte outside the region written";
    if (ok && R[0].L.o - kO0 > cap) ok = false, why = "more bytes than the bound";
    if (ok && nb % 8 == 0) {
        std::vector<uint8_t> by(nb / 8 + 1, 0), ref(cap + 64);
        for (uint32_t i = 0; i < nb; ++i) by[i >> 3] |= lit.b[i] << (7 - (i & 7));
        size_t rl = 0;
        const int rs = oracle_decode(by.data(), nb / 8, ref.data(), ref.size(), &rl);
        for (int d = 0; ok && d < 3; ++d)
            if (rs != (int)lit12_status(R[d].L) || rl != R[d].L.o - kO0 || memcmp(ref.data(), R[d].img + kO0, rl) != 0)
                ok = false, why = "not the oracle's result";
        ++g_oracle;
    }
    if (!ok) {
        if (g_bad < 10) printf("%s: %u bits at X %% 32 = %u: %s\n", what, nb, (P + 31u) & 31u, why);
        ++g_bad;
    }
    ++g_cases;
}

// codes of <= 13 bits (mostly 5..8) taking exactly `bits` bits; false if no such sequence was found
static bool fill_exact(Bits& B, uint32_t bits) {
    for (int tries = 0; tries < 200; ++tries) {
        Bits C = B;
        uint32_t got = 0;
        while (got < bits) {
            const uint32_t l = rng() % 8 ? 5 + rng() % 4 : 5 + rng() % 9;
            if (by_len[l].empty() || got + l > bits) {
                if (bits - got < 5) break;
                continue;
            }
            C.code(C.any(l));
            got += l;
        }
        if (got == bits) {
            B = C;
            return true;
        }
    }
    return false;
}

static void sweep(int per_rem) {  // (a)
    for (uint32_t rem = 0; rem <= kMin + kSteps * 2 * kBits + kBits; ++rem)
        for (int i = 0; i < per_rem; ++i) {
            Bits B;
            const uint32_t pad = std::min<uint32_t>(rem, rng() % 8);
            if (fill_exact(B, rem - pad))
                B.ones(pad);
            else
                B.ones(rem);  // (no sequence of codes takes 1..4 or 9 bits)
            for (uint32_t al = 0; al < 32; ++al) one_case(B, al, "sweep");
        }
}

static void long_codes(int stride) {  // (b)
    for (int s = HPK_NSYM - 1; s >= 0; s -= stride) {
        const uint32_t len = T.len[s];
        if (len <= kBits) continue;
        for (int step = 0; step < kSteps; ++step)
            for (int second = 0; second < 2; ++second) {
                Bits pre;
                for (int c = 0; c < 2 * step + second; ++c) pre.code(pre.any(7));
                for (int suf = 0; suf <= 4; ++suf) {  // it fits
                    Bits B = pre;
                    B.code(s);
                    for (int c = 0; c < suf; ++c) B.code(B.any(suf & 1 ? 7 : 5 + rng() % 4));
                    B.pad();
                    for (uint32_t al = 0; al < 32; al += 1 + (uint32_t)suf) one_case(B, al, "long code");
                }
                for (uint32_t r = 18; r < len; ++r) {  // cut by the literal's end
                    Bits B = pre;
                    B.put(T.code[s] >> (len - r), r);
                    for (uint32_t k = 0; k < 4; ++k) one_case(B, (r * 5u + 8u * k + (uint32_t)s) & 31u, "cut long code");
                }
            }
    }
}

static void two_long(int n) {  // (c)
    std::vector<int> longs;
    for (int s = 0; s < HPK_NSYM; ++s)
        if (T.len[s] > kBits) longs.push_back(s);
    for (int i = 0; i < n; ++i) {
        Bits B;
        const int p = i % 6, q = (i / 6) % 3;
        for (int c = 0; c < p; ++c) B.code(B.any(7));
        B.code(longs[rng() % longs.size()]);
        for (int c = 0; c < q; ++c) B.code(B.any(7));
        B.code(longs[rng() % (longs.size() - 1)]);  // (not EOS, the last symbol: the walk goes on)
        for (int c = 0; c < 3; ++c) B.code(B.any(5 + rng() % 4));
        B.pad();
        one_case(B, (uint32_t)rng() & 31u, "two long codes");
    }
}

static void exact_end(int stride) {  // (d)
    for (int s = 255; s >= 0; s -= stride) {
        const uint32_t b = T.len[s];
        if (b <= kBits) continue;
        for (uint32_t a = 5; a <= kBits; ++a) {
            if (by_len[a].empty() || a + b < kMin) continue;
            for (int k = 0; k < kSteps; ++k) {
                Bits B;
                for (int c = 0; c < 2 * k; ++c) B.code(B.any(7));
                B.code(B.any((int)a));
                B.code(s);
                for (uint32_t al = 0; al < 32; al += 3) one_case(B, al, "exact end");
            }
        }
    }
}

static void mix(int n) {  // (e)
    const char* text = "abcdefghijklmnopqrstuvwxyz0123456789-_=;,/.:ABC ";
    for (int i = 0; i < n; ++i) {
        const int kind = (int)(rng() % 8), len = (int)(rng() % 61);
        std::vector<uint8_t> s(len);
        for (auto& c : s) c = kind <= 1 ? (uint8_t)text[rng() % strlen(text)] : (uint8_t)rng();
        std::vector<uint8_t> enc(4 * len + 8);
        if (kind <= 2 || kind >= 6) {
            size_t el = 0;
            oracle_encode(s.data(), s.size(), enc.data(), enc.size(), &el);
            enc.resize(el);
        } else {
            enc = s;  // random bytes: padding errors, EOS, long codes
        }
        if (kind == 4 && enc.size() > 2) enc[enc.size() - 1] &= 0xF0;
        if (kind == 5 && enc.size() > 4) {
            const size_t p = rng() % (enc.size() - 3);
            enc[p] = enc[p + 1] = enc[p + 2] = enc[p + 3] = 0xFF;
        }
        if (kind == 7) enc.push_back(0xFF);  // too much padding
        Bits B;
        for (uint8_t c : enc) B.put(c, 8);
        one_case(B, (uint32_t)rng() & 31u, "mix");
    }
}

int main(int argc, char** argv) {
    if (hpk_build_tables(&T)) {
        printf("table build failed\n");
        return 1;
    }
    const int seed = argc > 1 ? atoi(argv[1]) : 1;
    const int scale = argc > 2 ? atoi(argv[2]) : 8;
    const int stride = argc > 3 ? atoi(argv[3]) : 1;  // (b), (d): every stride-th symbol (a sanitizer build's run)
    rng.seed(seed);
    for (int s = 0; s < 256; ++s) by_len[T.len[s]].push_back(s);
    sweep(scale);
    printf("sweep: %ld cases, first round of", g_cases);
    for (int j = 0; j <= kSteps; ++j) printf(" %ld", g_first[j]);
    printf(" steps\n");
    long c0 = g_cases;
    long_codes(stride);
    printf("long codes: %ld cases, in the body at", g_cases - c0);
    for (int j = 0; j < kSteps; ++j) printf(" %ld %ld", g_place[j][0], g_place[j][1]);
    printf(", %ld PaddingTooLarge, %ld EOSInString\n", g_ptl, g_eos);
    c0 = g_cases;
    two_long(500 * scale);
    printf("two long codes: %ld cases, %ld rounds with two\n", g_cases - c0, g_two);
    c0 = g_cases;
    const long e0 = g_exact;
    exact_end(stride);
    printf("exact end: %ld cases, %ld steps ended a literal exactly\n", g_cases - c0, g_exact - e0);
    c0 = g_cases;
    mix(5000 * scale);
    printf("mix: %ld cases\n", g_cases - c0);
    printf("parked lanes by step:");
    for (int j = 0; j < kSteps; ++j) printf(" %ld", g_parked[j]);
    printf("\n");
    printf("total: %ld cases, %ld rounds, %ld literals against the oracle\n", g_cases, g_rounds, g_oracle);
    printf("%s: %ld mismatches\n", g_bad ? "FAIL" : "ok", g_bad);
    return g_bad != 0;
}
