// hpk_chunks.h — how a host-pointer batch (hpk_calls_batch.hip, host_begin) is cut into the literal ranges its
// pipeline copies in, runs and copies out one after another. Host arithmetic only, no HIP header:
// tests/emu/chunks_emu.cpp builds it with g++, and tests/host_chunk_cases.py restates it in Python.
#pragma once
#include <stddef.h>
#include <stdint.h>

static constexpr int kHpkMaxChunks = 8;                        // the most ranges one call is cut into
static constexpr size_t kHpkChunkBytes = (size_t)4 << 20;      // bytes moved (in and out) that are worth a range

// The number of ranges: one per kHpkChunkBytes of input and output bytes together, at least 1, at most
// kHpkMaxChunks and at most one per literal (so 0 for an empty batch).
static inline int hpk_chunk_count(size_t in_bytes, size_t out_bytes, uint32_t n) {
    const size_t want = (in_bytes + out_bytes) / kHpkChunkBytes;
    int chunks = want < 1 ? 1 : (want > (size_t)kHpkMaxChunks ? kHpkMaxChunks : (int)want);
    if ((uint32_t)chunks > n) chunks = (int)n;
    return chunks;
}

// cut[0 .. chunks]: range j is the literals [cut[j], cut[j + 1]), balanced by encoded bytes (in_bytes = in_off[n]):
// cut[j] is the first literal whose end passes j/chunks of the bytes. cut[] has room for kHpkMaxChunks + 1
// entries; returns the number of ranges. Ranges may be empty (one literal holding most of the bytes).
static inline int hpk_chunk_cuts(const uint32_t* in_off, uint32_t n, size_t out_bytes, uint32_t* cut) {
    const size_t in_bytes = in_off[n];
    const int chunks = hpk_chunk_count(in_bytes, out_bytes, n);
    cut[0] = 0;
    for (int j = 1; j < chunks; ++j) {
        const uint64_t target = (uint64_t)in_bytes * j / chunks;
        uint32_t lo = cut[j - 1], hi = n;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (in_off[mid + 1] < target) lo = mid + 1; else hi = mid;
        }
        cut[j] = lo;
    }
    cut[chunks] = n;
    return chunks;
}
