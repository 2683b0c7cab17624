// hpk_hpack.h — what the block decoder (hpk_hdec.cpp) and the block encoder (hpk_henc.cpp) share: RFC 7541's
// static table and the grouping of a call's blocks by the decoder or encoder they belong to. Host code only, not
// part of the C ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string_view>
#include <unordered_map>
#include <vector>

// RFC 7541 Appendix A (the reference keeps it as STATIC_TABLE, crates/loona-hpack/src/lib.rs): entry i's name is
// hpk_static[i][0], its value hpk_static[i][1] (the lengths are the compiler's).
static constexpr std::string_view hpk_static[61][2] = {
    {":authority", ""},
    {":method", "GET"},
    {":method", "POST"},
    {":path", "/"},
    {":path", "/index.html"},
    {":scheme", "http"},
    {":scheme", "https"},
    {":status", "200"},
    {":status", "204"},
    {":status", "206"},
    {":status", "304"},
    {":status", "400"},
    {":status", "404"},
    {":status", "500"},
    {"accept-charset", ""},
    {"accept-encoding", "gzip, deflate"},
    {"accept-language", ""},
    {"accept-ranges", ""},
    {"accept", ""},
    {"access-control-allow-origin", ""},
    {"age", ""},
    {"allow", ""},
    {"authorization", ""},
    {"cache-control", ""},
    {"content-disposition", ""},
    {"content-encoding", ""},
    {"content-language", ""},
    {"content-length", ""},
    {"content-location", ""},
    {"content-range", ""},
    {"content-type", ""},
    {"cookie", ""},
    {"date", ""},
    {"etag", ""},
    {"expect", ""},
    {"expires", ""},
    {"from", ""},
    {"host", ""},
    {"if-match", ""},
    {"if-modified-since", ""},
    {"if-none-match", ""},
    {"if-range", ""},
    {"if-unmodified-since", ""},
    {"last-modified", ""},
    {"link", ""},
    {"location", ""},
    {"max-forwards", ""},
    {"proxy-authenticate", ""},
    {"proxy-authorization", ""},
    {"range", ""},
    {"referer", ""},
    {"refresh", ""},
    {"retry-after", ""},
    {"server", ""},
    {"set-cookie", ""},
    {"strict-transport-security", ""},
    {"transfer-encoding", ""},
    {"user-agent", ""},
    {"vary", ""},
    {"via", ""},
    {"www-authenticate", ""},
};

// A call's blocks by their owner (block b belongs to owner[b], a decoder or an encoder): the distinct owners in
// order of first appearance, and each one's blocks in call order.
template <class T>
struct hpk_groups {
    std::vector<T*> who;             // the distinct owners
    std::vector<uint32_t> of;        // block b belongs to who[of[b]]
    std::vector<uint32_t> off, list;  // who[k]'s blocks: list[off[k] .. off[k + 1])
};
template <class T>
static inline hpk_groups<T> hpk_group_blocks(T* const* owner, uint32_t nblocks) {
    hpk_groups<T> g;
    std::unordered_map<const T*, uint32_t> ids;
    g.of.resize(nblocks);
    for (uint32_t b = 0; b < nblocks; ++b) {
        if (b && owner[b] == owner[b - 1]) {  // (a connection's blocks tend to come together)
            g.of[b] = g.of[b - 1];
            continue;
        }
        const auto it = ids.try_emplace(owner[b], (uint32_t)g.who.size());  // (looks up before it allocates a node)
        if (it.second) g.who.push_back(owner[b]);
        g.of[b] = it.first->second;
    }
    g.off.assign(g.who.size() + 1, 0u);  // a counting pass, then the lists
    for (uint32_t b = 0; b < nblocks; ++b) g.off[g.of[b] + 1] += 1u;
    for (size_t k = 0; k < g.who.size(); ++k) g.off[k + 1] += g.off[k];
    g.list.resize(nblocks);
    std::vector<uint32_t> at(g.off.begin(), g.off.end() - 1);
    for (uint32_t b = 0; b < nblocks; ++b) g.list[at[g.of[b]]++] = b;
    return g;
}
