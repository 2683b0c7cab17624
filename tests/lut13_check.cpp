// Host check of the wave kernel's 13-bit two-symbol table (hpk_code.h, lut13: the LUT3 layout at
// HPK_LUT13_BITS index bits). Every one of the 8,192 prefixes is decoded again here by brute force from the
// 257 code lengths alone (the canonical codes are rebuilt here, not taken from the builder), and each field of
// the entry is compared: symbols, bits held, codes held, len0, the not-two flag. Also: an entry holding two
// codes holds <= 13 bits, and no prefix that starts with a code of <= 13 bits has an empty entry.
// Prints "ok" and the counts, or the first mismatch. Built and run by tests/test_lut13.py.
#include <cstdio>

#include "hpk_code.h"

static unsigned g_code[HPK_NSYM];

static void canonical() {  // codes in (length, symbol) order
    unsigned long long c = 0;
    int prev = 0;
    bool first = true;
    for (int L = 1; L <= 30; ++L)
        for (int s = 0; s < HPK_NSYM; ++s)
            if (HPK_CODE_LEN[s] == L) {
                if (!first) c = (c + 1) << (L - prev);
                first = false;
                prev = L;
                g_code[s] = (unsigned)c;
            }
}

// the symbol whose code prefixes the nbits-bit string `bits` (MSB first) and fits in it; EOS (256) counts
static int first_code(unsigned bits, int nbits, int& sym, int& len) {
    for (int s = 0; s < HPK_NSYM; ++s) {
        const int L = HPK_CODE_LEN[s];
        if (L <= nbits && (bits >> (nbits - L)) == g_code[s]) {
            sym = s;
            len = L;
            return 1;
        }
    }
    return 0;
}

int main() {
    static hpk_tables t;
    if (hpk_build_tables(&t) != 0) {
        puts("table build failed");
        return 1;
    }
    canonical();
    const int B = HPK_LUT13_BITS;
    unsigned n0 = 0, n1 = 0, n2 = 0, n13 = 0;
    for (unsigned v = 0; v < HPK_LUT13_SIZE; ++v) {
        const unsigned e = t.lut13[v];
        int s0 = -1, l0 = 0, s1 = -1, l1 = 0;
        const int has0 = first_code(v, B, s0, l0) && s0 < 256;
        int has1 = 0;
        if (has0 && B - l0 >= 5) has1 = first_code(v & ((1u << (B - l0)) - 1u), B - l0, s1, l1) && s1 < 256;
        const unsigned codes = has0 ? (has1 ? 2u : 1u) : 0u;
        const unsigned held = has0 ? (unsigned)(l0 + (has1 ? l1 : 0)) : 0u;
        const unsigned want_len0 = has0 ? (unsigned)l0 : 15u;
        int ok = HPK_L3_CODES(e) == codes && HPK_L3_HELD(e) == held && HPK_L3_LEN0(e) == want_len0 &&
                 ((e >= HPK_L3_NOTTWO) == (codes < 2u)) && (!has0 || (e & 0xFFu) == (unsigned)s0) &&
                 (!has1 || ((e >> 16) & 0xFFu) == (unsigned)s1) && (e & 0x40000000u) == 0u;
        ok = ok && held <= (unsigned)B && (codes != 2u || HPK_L3_HELD(e) <= 13u);  // two codes: <= 13 bits held
        ok = ok && !(has0 && HPK_L3_CODES(e) == 0u);                               // a first code of <= 13 bits: not empty
        ok = ok && want_len0 != 14u && 15u > HPK_LUT2_CLAMP && (unsigned)B < HPK_LUT2_CLAMP;  // the checked step's compares
        if (!ok) {
            printf("entry %u = %08x: codes %u held %u len0 %u sym0 %d sym1 %d\n", v, e, codes, held, want_len0, s0, s1);
            return 1;
        }
        n0 += codes == 0u;
        n1 += codes == 1u;
        n2 += codes == 2u;
        n13 += codes == 2u && held == 13u;
    }
    printf("ok %u entries: %u empty, %u of one code, %u of two (%u holding 13 bits)\n", (unsigned)HPK_LUT13_SIZE, n0, n1, n2, n13);
    return 0;
}
