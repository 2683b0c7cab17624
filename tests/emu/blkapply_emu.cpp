// host replay of the header-block apply (loona_amd/csrc/hpk_blkapply.hip): the REAL per-record code of
// hpk_blkapply.h (check_record, stage_record, apply_record, finish_block) over a table that is a plain array ring,
// one decoder at a time, on decoders read from a file that tests/test_blkapply_emulation.py writes (and whose
// answers it takes from blocks_apply_cases.ref_apply). The program lays out the arena as a caller of
// hpk_apply_blocks would (the static text, the carried-in entries' bytes, the packed strings), walks a decoder's
// records as the kernel does (the look over all of them first, then chunks of 64 staged before they are applied in
// order) and prints every reference resolved to bytes, so the comparison is on names and values.
//   usage: blkapply_emu <cases file> <ring records (a power of two)>
//   file (u32 words and raw bytes): 61 static entries (nl, vl, bytes); the decoder count; per decoder max_size,
//   max_allowed, cap, count, the entries (nl, vl, bytes; newest first), the block count, per block the field count
//   and the hpk_field records (index, str, kind | nstr << 8 | err << 16 | err_stage << 24, at; str counted over the
//   decoder's blocks), then the decoder's string count and per string status, length, bytes
//   output: per block "B n_headers error detail" and " name:value" in hex per header; per decoder
//   "T applied count size max_size" and its entries, newest first
#include "shim.h"
#include "hpk_blkapply.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

using namespace hpkapp;

struct ArrayRing {
    std::vector<hpk_header> ring;
    uint32_t head, count, size, max_size, max_allowed;
    hpk_header get(uint32_t i) const { return ring[(head + i) & (ring.size() - 1)]; }
    void push(const hpk_header& h) {
        head = (head - 1u) & (uint32_t)(ring.size() - 1);
        ring[head] = h;
        count += 1u;
    }
    void pop() { count -= 1u; }
    void clear() { count = 0u; }
};

static FILE* g_f;
static uint32_t u32() {
    uint32_t v = 0;
    if (fread(&v, 4, 1, g_f) != 1) exit(2);
    return v;
}
static void bytes(std::vector<uint8_t>& to, uint32_t n) {
    const size_t at = to.size();
    to.resize(at + n);
    if (n && fread(to.data() + at, 1, n, g_f) != n) exit(2);
}

static void hex(const std::vector<uint8_t>& arena, uint32_t off, uint32_t len) {
    if ((uint64_t)off + len > arena.size()) {
        printf("!outside");
        return;
    }
    for (uint32_t i = 0; i < len; ++i) printf("%02x", arena[off + i]);
}
static void put(const std::vector<uint8_t>& arena, const hpk_header& h) {
    printf(" ");
    hex(arena, h.name_off, h.name_len);
    printf(":");
    hex(arena, h.value_off, h.value_len);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    g_f = fopen(argv[1], "rb");
    if (!g_f) return 2;
    const uint32_t ring = (uint32_t)atoi(argv[2]);
    if (!ring || (ring & (ring - 1u))) return 2;
    const uint32_t static_base = 16u;
    std::vector<uint8_t> stat_text(static_base, 0xEE);
    hpk_header stat[61];
    for (int k = 0; k < 61; ++k) {
        const uint32_t nl = u32(), vl = u32();
        stat[k] = hpk_header{(uint32_t)stat_text.size() - static_base, nl, (uint32_t)stat_text.size() - static_base + nl, vl};
        bytes(stat_text, nl + vl);
    }
    const uint32_t ndecs = u32();
    for (uint32_t d = 0; d < ndecs; ++d) {
        std::vector<uint8_t> arena = stat_text;
        arena.resize(arena.size() + 5, 0xEE);
        ArrayRing t{std::vector<hpk_header>(ring), 0u, 0u, 0u, 0u, 0u};
        t.max_size = u32();
        t.max_allowed = u32();
        const uint32_t cap = u32(), count0 = u32();
        std::vector<hpk_header> ent(count0);
        for (uint32_t i = 0; i < count0; ++i) {
            const uint32_t nl = u32(), vl = u32();
            ent[i] = hpk_header{(uint32_t)arena.size(), nl, (uint32_t)arena.size() + nl, vl};
            bytes(arena, nl + vl);
            t.size += nl + vl + 32u;
        }
        const uint32_t nblocks = u32();
        std::vector<std::vector<uint32_t>> fields(nblocks);
        for (uint32_t b = 0; b < nblocks; ++b) {
            fields[b].resize(4 * (size_t)u32());
            for (uint32_t& w : fields[b]) w = u32();
        }
        const uint32_t nstrs = u32();
        arena.resize(arena.size() + 3, 0xEE);
        const uint32_t str_base = (uint32_t)arena.size();
        std::vector<uint32_t> out_off(nstrs + 1, 0u), out_len(nstrs, 0u);
        std::vector<uint8_t> status(nstrs, 0);
        for (uint32_t s = 0; s < nstrs; ++s) {
            status[s] = (uint8_t)u32();
            out_len[s] = u32();
            out_off[s] = (uint32_t)arena.size() - str_base;
            bytes(arena, out_len[s]);
        }
        // the look
        const uint32_t lim = cap < ring ? cap : ring, limit = 32u * lim;
        uint32_t kdef = nblocks;
        bool bad = count0 > cap;
        for (uint32_t b = 0; b < nblocks; ++b) {
            bool big = false;
            for (size_t i = 0; i < fields[b].size(); i += 4) {
                bool bg;
                bad |= !check_record(fields[b][i], fields[b][i + 1], fields[b][i + 2], out_off.data(), out_len.data(), nstrs,
                                     str_base, limit, &bg);
                big |= bg;
            }
            if (big && kdef == nblocks) kdef = b;
        }
        if (bad) {
            printf("V\n");
            continue;
        }
        const uint32_t napply = (t.max_size > limit || count0 > lim) ? 0u : kdef;
        if (napply) {
            for (uint32_t i = 0; i < count0; ++i) t.ring[i] = ent[i];
            t.count = count0;
        }
        for (uint32_t b = 0; b < nblocks; ++b) {
            if (b >= napply) {
                printf("B 0 %d 0\n", HPK_BLK_DEFERRED);
                continue;
            }
            Blk blk = {0u, 0, 0, 0u};
            std::vector<hpk_header> hs;
            bool stopped = false;
            const size_t nf = fields[b].size() / 4;
            for (size_t c = 0; c < nf && !stopped; c += 64) {
                const size_t nrec = nf - c < 64 ? nf - c : 64;
                Rec r[64];
                for (size_t i = 0; i < nrec; ++i) {
                    const uint32_t* f = &fields[b][4 * (c + i)];
                    r[i] = stage_record(f[0], f[1], f[2], out_off.data(), out_len.data(), status.data(), str_base);
                }
                for (size_t i = 0; i < nrec; ++i) {
                    hpk_header h;
                    const Step s = apply_record(t, stat, static_base, r[i], blk, &h);
                    if (s == kStop) {
                        stopped = true;
                        break;
                    }
                    if (s == kEmit) hs.push_back(h);
                }
            }
            if (!stopped) finish_block(blk);
            if (hs.size() != blk.n_headers) printf("# block %u: %zu headers emitted, %u counted\n", b, hs.size(), blk.n_headers);
            printf("B %u %d %d", blk.n_headers, blk.error, blk.detail);
            for (const hpk_header& h : hs) put(arena, h);
            printf("\n");
        }
        if (!napply) {  // untouched: the entries as they came
            printf("T 0 %u %u %u", count0, t.size, t.max_size);
            for (const hpk_header& h : ent) put(arena, h);
        } else {
            printf("T %u %u %u %u", napply, t.count, t.size, t.max_size);
            if (t.count > lim) printf(" !count above lim");
            for (uint32_t i = 0; i < t.count && i < ring; ++i) put(arena, t.get(i));
        }
        printf("\n");
    }
    fclose(g_f);
    printf("done: %u decoders\n", ndecs);
    return 0;
}
