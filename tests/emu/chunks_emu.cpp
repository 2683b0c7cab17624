// chunks_emu.cpp — prints what the REAL hpk_chunks.h answers for the argument tuples on its standard input, one per
// line:
//   "count <in_bytes> <out_bytes> <n>"                       -> "count <chunks>"
//   "cuts <out_bytes> <n> <in_off[0]> ... <in_off[n]>"       -> "cuts <chunks> <cut[0]> ... <cut[chunks]>"
// and first of all one line "consts <kHpkMaxChunks> <kHpkChunkBytes>". tests/test_host_chunk_cases.py compares
// them with the Python model of tests/host_chunk_cases.py.
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "hpk_chunks.h"

int main() {
    printf("consts %d %zu\n", kHpkMaxChunks, kHpkChunkBytes);
    std::string line;
    int lines = 0;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "count") {
            unsigned long long in_bytes, out_bytes, n;
            if (!(in >> in_bytes >> out_bytes >> n)) return 2;
            printf("count %d\n", hpk_chunk_count((size_t)in_bytes, (size_t)out_bytes, (uint32_t)n));
        } else if (what == "cuts") {
            unsigned long long out_bytes, n, x;
            if (!(in >> out_bytes >> n)) return 2;
            std::vector<uint32_t> off;  // exactly n + 1 entries: a read past them is the sanitizer's to report
            while (in >> x) off.push_back((uint32_t)x);
            if (off.size() != n + 1) return 2;
            std::vector<uint32_t> cut(kHpkMaxChunks + 1, 0xFFFFFFFFu);
            const int chunks = hpk_chunk_cuts(off.data(), (uint32_t)n, (size_t)out_bytes, cut.data());
            printf("cuts %d", chunks);
            for (int j = 0; j <= chunks; ++j) printf(" %u", cut[j]);
            for (int j = chunks + 1; j <= kHpkMaxChunks; ++j)
                if (cut[j] != 0xFFFFFFFFu) return 3;  // nothing written behind cut[chunks]
            printf("\n");
        } else {
            printf("?\n");
            return 2;
        }
        ++lines;
    }
    fprintf(stderr, "ok: %d tuples\n", lines);
    return 0;
}
