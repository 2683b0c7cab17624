// host replay of the header-block plan (loona_amd/csrc/hpk_blkplan.hip): the REAL per-header code of hpk_blkplan.h
// (hash, test_entry, combine, build, check_header, check_entry) and hpk_blkapply.h's insert over a table that is a
// plain array ring, one encoder at a time, on encoders read from a file that tests/test_blkplan_emulation.py writes
// (and whose answers it takes from blocks_plan_cases.ref_plan). The program lays out the arena as a caller of
// hpk_plan_blocks would (the static text, the carried-in entries' bytes, the fields, the prefix area), walks an
// encoder as the kernel does (the look, the table hashed at load, chunks of 64 headers staged before they are
// resolved in order, the search in groups of 64 entries with the 64 lanes run in a loop and their answers gathered
// into the two ballots) and prints every reference resolved to bytes.
//   usage: blkplan_emu <cases file> <ring records (a power of two)>
//   file (u32 words and raw bytes): 61 static entries (nl, vl, bytes); the encoder count; per encoder max_size, cap,
//   huffman, count, the entries (nl, vl, bytes; newest first), the block count, per block the header count and the
//   headers (nl, vl, bytes)
//   output: per block "B" and per header " kind,index,prefix,policy:bytes,policy:bytes,policy:bytes" in hex, or "D"
//   for a deferred block; per encoder "T planned count size max_size" and its entries, newest first
#include "shim.h"
#include "hpk_blkplan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

using namespace hpkplan;

struct ArrayRing {
    std::vector<Ent> ring;
    uint32_t head, count, size, max_size, nh, vh;
    hpk_header get(uint32_t i) const { return ring[(head + i) & (ring.size() - 1)].h; }
    const Ent& ent(uint32_t i) const { return ring[(head + i) & (ring.size() - 1)]; }
    void push(const hpk_header& h) {
        head = (head - 1u) & (uint32_t)(ring.size() - 1);
        ring[head] = Ent{h, nh, vh};
        count += 1u;
    }
    void pop() { count -= 1u; }
    void clear() { count = 0u; }
};

struct VecBytes {
    const std::vector<uint8_t>* v;
    uint32_t operator()(uint32_t at) const {
        if (at >= v->size()) {
            printf("!read outside the arena\n");
            return 0;
        }
        return (*v)[at];
    }
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
    const uint32_t nencs = u32();
    for (uint32_t e = 0; e < nencs; ++e) {
        std::vector<uint8_t> arena = stat_text;
        arena.resize(arena.size() + 5, 0xEE);
        ArrayRing t{std::vector<Ent>(ring), 0u, 0u, 0u, 0u, 0u, 0u};
        t.max_size = u32();
        const uint32_t cap = u32(), huffman = u32(), count0 = u32();
        std::vector<hpk_header> ent(count0);
        for (uint32_t i = 0; i < count0; ++i) {
            const uint32_t nl = u32(), vl = u32();
            ent[i] = hpk_header{(uint32_t)arena.size(), nl, (uint32_t)arena.size() + nl, vl};
            bytes(arena, nl + vl);
            t.size += nl + vl + 32u;
        }
        arena.resize(arena.size() + 3, 0xEE);
        const uint32_t fields_base = (uint32_t)arena.size();
        const uint32_t nblocks = u32();
        std::vector<uint32_t> hdr_off(1, 0u), field_off(1, 0u);
        for (uint32_t b = 0; b < nblocks; ++b) {
            const uint32_t nh = u32();
            for (uint32_t j = 0; j < nh; ++j) {
                const uint32_t nl = u32(), vl = u32();
                bytes(arena, nl + vl);
                field_off.push_back(field_off.back() + nl);
                field_off.push_back(field_off.back() + vl);
            }
            hdr_off.push_back(hdr_off.back() + nh);
        }
        const uint32_t nh_all = hdr_off.back();
        arena.resize((arena.size() + 3) & ~(size_t)3, 0xEE);
        const uint32_t prefix_base = (uint32_t)arena.size();
        arena.resize(arena.size() + 4 * (size_t)nh_all, 0xEE);
        const uint64_t arena_cap = arena.size();
        const VecBytes by{&arena};
        // the first pass: the hashes (the defaults are what a header that is never resolved prints)
        std::vector<uint32_t> hn(nh_all), hv(nh_all);
        for (uint32_t j = 0; j < nh_all; ++j) {
            hn[j] = hash(by, fields_base + field_off[2 * j], field_off[2 * j + 1] - field_off[2 * j]);
            hv[j] = hash(by, fields_base + field_off[2 * j + 1], field_off[2 * j + 2] - field_off[2 * j + 1]);
        }
        // the look
        bool bad = count0 > cap;
        for (uint32_t j = 0; j < nh_all; ++j)
            bad |= !check_header(field_off[2 * j], field_off[2 * j + 1], field_off[2 * j + 2], fields_base, arena_cap);
        for (uint32_t i = 0; i < count0; ++i) bad |= !check_entry(ent[i], arena_cap);
        if (bad) {
            printf("V\n");
            continue;
        }
        const uint32_t lim = cap < ring ? cap : ring;
        if (t.max_size > 32u * lim || count0 > lim) {
            for (uint32_t b = 0; b < nblocks; ++b) printf("D\n");
            printf("T 0 %u %u %u", count0, t.size, t.max_size);
            for (const hpk_header& h : ent) {
                printf(" ");
                hex(arena, h.name_off, h.name_len);
                printf(":");
                hex(arena, h.value_off, h.value_len);
            }
            printf("\n");
            continue;
        }
        for (uint32_t i = 0; i < count0; ++i)
            t.ring[i] = Ent{ent[i], hash(by, ent[i].name_off, ent[i].name_len), hash(by, ent[i].value_off, ent[i].value_len)};
        t.count = count0;
        Ent se[64];
        for (uint32_t l = 0; l < kStaticEntries; ++l) {
            se[l].h = stat[l];
            se[l].h.name_off += static_base;
            se[l].h.value_off += static_base;
            se[l].nh = hash(by, se[l].h.name_off, se[l].h.name_len);
            se[l].vh = hash(by, se[l].h.value_off, se[l].h.value_len);
        }
        const uint32_t policy = huffman ? HPK_STR_AUTO : HPK_STR_RAW;
        for (uint32_t b = 0; b < nblocks; ++b) {
            printf("B");
            for (uint32_t c = hdr_off[b]; c < hdr_off[b + 1]; c += 64u) {
                const uint32_t nrec = hdr_off[b + 1] - c < 64u ? hdr_off[b + 1] - c : 64u;
                Ent q[64];
                for (uint32_t l = 0; l < nrec; ++l) {
                    const uint32_t j = c + l, f0 = field_off[2 * j], f1 = field_off[2 * j + 1], f2 = field_off[2 * j + 2];
                    q[l] = Ent{hpk_header{fields_base + f0, f1 - f0, fields_base + f1, f2 - f1}, hn[j], hv[j]};
                }
                Out mine[64];
                for (uint32_t i = 0; i < nrec; ++i) {
                    const Ent u = q[i];
                    Found f = {0u, 0u};
                    uint64_t full = 0, name = 0;
                    for (uint32_t l = 0; l < kStaticEntries; ++l) {
                        const Match m = test_entry(by, se[l], u);
                        full |= (uint64_t)(m == kFull) << l;
                        name |= (uint64_t)(m != kNone) << l;
                    }
                    bool done = combine(full, name, 1u, f);
                    for (uint32_t g = 0; !done && g < t.count; g += kGroup) {
                        full = name = 0;
                        for (uint32_t l = 0; l < 64u && g + l < t.count; ++l) {
                            const Match m = test_entry(by, t.ent(g + l), u);
                            full |= (uint64_t)(m == kFull) << l;
                            name |= (uint64_t)(m != kNone) << l;
                        }
                        done = combine(full, name, kStaticEntries + 1u + g, f);
                    }
                    mine[i] = build(f, u.h, policy, prefix_base + 4u * (c + i));
                    if (kind_of(f) == HPK_PLAN_NEW_NAME) {
                        t.nh = u.nh;
                        t.vh = u.vh;
                        hpkapp::insert(t, u.h);
                    }
                }
                for (uint32_t l = 0; l < nrec; ++l) {
                    const Out& o = mine[l];
                    memcpy(&arena[prefix_base + 4u * (c + l)], &o.prefix, 4);
                    const uint32_t plen = (o.rep[1] >> 8) & 255u;
                    printf(" %u,%u,", o.rep[1] & 255u, o.rep[0]);
                    for (uint32_t k = 0; k < plen; ++k) printf("%02x", (o.rep[2] >> (8 * k)) & 255u);
                    for (uint32_t k = 0; k < 3u; ++k) {
                        printf(",%u:", o.pol[k]);
                        hex(arena, o.off[k], o.len[k]);
                    }
                }
            }
            printf("\n");
        }
        printf("T %u %u %u %u", nblocks, t.count, t.size, t.max_size);
        if (t.count > lim) printf(" !count above lim");
        for (uint32_t i = 0; i < t.count && i < ring; ++i) {
            printf(" ");
            hex(arena, t.get(i).name_off, t.get(i).name_len);
            printf(":");
            hex(arena, t.get(i).value_off, t.get(i).value_len);
        }
        printf("\n");
    }
    fclose(g_f);
    printf("done: %u encoders\n", nencs);
    return 0;
}
