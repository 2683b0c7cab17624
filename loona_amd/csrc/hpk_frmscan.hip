// hpk_frmscan.hip — the HTTP/2 frame scan's own kernels (hpk_scan_frames, hpk_frame_blocks): step 1 of
// hpk_h2_read_frames on many connections at once. A translation unit of its own. The call's steps
// (hpk_calls_frames.hip strings them together):
//   * hpk_frmcount below, one lane per connection (per-lane code in hpk_frmscan.h): the connection's completed
//     blocks, its closed fragments (those of the completed blocks) and its open ones (the trailing fragments of a
//     block still pending at the end); a void connection counts 0 of each and sets the sticky flag. It does not
//     write the state: the emit pass still needs it as it came in;
//   * hpk_len_scan (hpk_pack.hip, as it is) over each count array: conn_blk_off, conn_frag_off, conn_open_off;
//   * hpk_frmemit below, one lane per connection again: the same walk with a visitor that stores every block
//     record (one 16-byte store) and every fragment window, closed or open, each only below the caller's capacity;
//     then the connection's state, consumed and status (two 16-byte stores);
//   * hpk_frmboff (hpk_frame_blocks, behind the ordered pack of the closed fragments): where each block's bytes
//     begin in the packed blob.
// The lanes read the connections with byte loads (hpk_frmscan.h says why). One lane walks one whole connection:
// a connection of many thousands of small frames costs two dependent loads per frame on that lane while its 255
// neighbours wait (include/hpk.h states it).
#include "hpk_device.h"
#include "hpk_frmscan.h"

namespace {

constexpr uint32_t kFrmWg = 256;  // connections per workgroup, one per lane (hpk_test_frmscan_geometry)

struct FrmArgs {
    const uint8_t* blob;
    uint32_t cap;
    const uint32_t* off;
    uint32_t nconn;
    uint4* conns;  // hpk_fconn as two 16-byte halves
    // the count pass's outputs
    uint32_t* nblk;
    uint32_t* nclosed;
    uint32_t* nopen;
    uint32_t* err;
    // the emit pass's inputs and outputs
    const uint32_t* conn_blk_off;
    const uint32_t* conn_frag_off;
    const uint32_t* conn_open_off;
    uint4* blocks;
    uint32_t blocks_cap;
    uint32_t* frag_off;
    uint32_t* frag_len;
    uint32_t frags_cap;
    uint32_t* open_off;
    uint32_t* open_len;
    uint32_t opens_cap;
};

__global__ __launch_bounds__(kFrmWg) void hpk_frmcount(FrmArgs a) {
    const uint32_t c = blockIdx.x * kFrmWg + threadIdx.x;
    if (c >= a.nconn) return;
    const uint32_t lo = a.off[c], hi = a.off[c + 1];
    const uint4 s0 = a.conns[2u * (size_t)c], s1 = a.conns[2u * (size_t)c + 1u];
    hpkfrm::Counts n = {0u, 0u, 0u, 0u};
    if (!hpkfrm::conn_ok(lo, hi, a.cap, s0.z, s1.x, s1.y)) {
        *a.err = 1u;
    } else {
        hpkfrm::State s{s0.x, (int32_t)s0.y, s0.z, s0.w};
        hpkfrm::NoVisit v;
        n = hpkfrm::walk_frames(a.blob, lo, hi, s, s1.x, s1.y, v);
    }
    a.nblk[c] = n.blocks;
    a.nclosed[c] = n.frags - n.open;
    a.nopen[c] = n.open;
}

struct EmitVisit {
    uint32_t conn;
    uint4* blocks;
    uint32_t bbase, blocks_cap;
    // the closed list's arrays, and how far behind them the open list's lie, in bytes. (One store site whose address
    // is the closed array's plus 0 or that distance: with a pointer per list, whether in two store sites or selected
    // at one, the compiler kept the four pointers as a table in scratch and indexed it.)
    uintptr_t frag_off, frag_len, open_off_d, open_len_d;
    uint32_t fbase, nclosed, frags_cap;
    uint32_t obase, opens_cap;
    // (bases and counts are sums of at most cap / 9 + nconn < 2^31 items: no wrap)
    __device__ __forceinline__ void fragment(uint32_t j, uint32_t off, uint32_t len) {
        const bool closed = j < nclosed;
        const uint32_t g = closed ? fbase + j : obase + (j - nclosed);
        if (g < (closed ? frags_cap : opens_cap)) {
            *reinterpret_cast<uint32_t*>(frag_off + (closed ? 0u : open_off_d) + 4u * (uintptr_t)g) = off;
            *reinterpret_cast<uint32_t*>(frag_len + (closed ? 0u : open_len_d) + 4u * (uintptr_t)g) = len;
        }
    }
    __device__ __forceinline__ void block(uint32_t k, uint32_t sid_es, uint32_t first, uint32_t nfrag) {
        const uint32_t g = bbase + k;
        if (g < blocks_cap) blocks[g] = make_uint4(conn, sid_es, fbase + first, nfrag);
    }
};

__global__ __launch_bounds__(kFrmWg) void hpk_frmemit(FrmArgs a) {
    const uint32_t c = blockIdx.x * kFrmWg + threadIdx.x;
    if (c >= a.nconn) return;
    const uint32_t lo = a.off[c], hi = a.off[c + 1];
    const uint4 s0 = a.conns[2u * (size_t)c], s1 = a.conns[2u * (size_t)c + 1u];
    if (!hpkfrm::conn_ok(lo, hi, a.cap, s0.z, s1.x, s1.y)) {  // void: the count pass has set the flag
        a.conns[2u * (size_t)c + 1u] = make_uint4(s1.x, s1.y, s1.z, HPK_BAD_OFFSETS);
        return;
    }
    hpkfrm::State s{s0.x, (int32_t)s0.y, s0.z, s0.w};
    const uint32_t fbase = a.conn_frag_off[c];
    const uintptr_t fo = (uintptr_t)a.frag_off, fl = (uintptr_t)a.frag_len;
    EmitVisit v{c,  a.blocks, a.conn_blk_off[c], a.blocks_cap, fo, fl, (uintptr_t)a.open_off - fo, (uintptr_t)a.open_len - fl, fbase,
                a.conn_frag_off[c + 1] - fbase, a.frags_cap, a.conn_open_off[c], a.opens_cap};
    const hpkfrm::Counts n = hpkfrm::walk_frames(a.blob, lo, hi, s, s1.x, s1.y, v);
    a.conns[2u * (size_t)c] = make_uint4(s.max_frame_size, (uint32_t)s.error, s.pending, s.pend_stream);
    a.conns[2u * (size_t)c + 1u] = make_uint4(s1.x, s1.y, n.consumed, HPK_OK);
}

// block_off[b] = dst_off[blocks[b].frag] for b < nblocks, block_off[nblocks] = dst_off[nfrags]; a record whose
// frag passes nfrags is read as nfrags, one below its predecessor's as the predecessor's (the sticky flag either way)
__global__ __launch_bounds__(kFrmWg) void hpk_frmboff(const uint32_t* dst_off, uint32_t nfrags, const uint4* blocks, uint32_t nblocks,
                                                        uint32_t* block_off, uint32_t* err) {
    const uint32_t b = blockIdx.x * kFrmWg + threadIdx.x;
    if (b > nblocks) return;
    uint32_t f = nfrags;
    if (b < nblocks) {
        f = blocks[b].z;
        bool bad = f > nfrags;
        if (bad) f = nfrags;
        if (b > 0u) {
            uint32_t p = blocks[b - 1u].z;
            if (p > nfrags) p = nfrags;
            if (f < p) {
                f = p;
                bad = true;
            }
        }
        if (bad) *err = 1u;
    }
    block_off[b] = dst_off[f];
}
}  // namespace

static_assert(sizeof(hpk_fconn) == 32 && sizeof(hpk_fblock) == 16, "hpk_fconn is two 16-byte stores, hpk_fblock one");

int hpk_launch_frmcount(hpk_ctx* c, const uint8_t* blob, uint32_t cap, const uint32_t* off, uint32_t nconn, const hpk_fconn* conns,
                        uint32_t* nblk, uint32_t* nclosed, uint32_t* nopen) {
    FrmArgs a{};
    a.blob = blob;
    a.cap = cap;
    a.off = off;
    a.nconn = nconn;
    a.conns = reinterpret_cast<uint4*>(const_cast<hpk_fconn*>(conns));
    a.nblk = nblk;
    a.nclosed = nclosed;
    a.nopen = nopen;
    a.err = c->d_err;
    hipLaunchKernelGGL(hpk_frmcount, dim3((nconn + kFrmWg - 1u) / kFrmWg), dim3(kFrmWg), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}

int hpk_launch_frmemit(hpk_ctx* c, const uint8_t* blob, uint32_t cap, const uint32_t* off, uint32_t nconn, hpk_fconn* conns,
                       const uint32_t* conn_blk_off, const uint32_t* conn_frag_off, const uint32_t* conn_open_off, hpk_fblock* blocks,
                       uint32_t blocks_cap, uint32_t* frag_off, uint32_t* frag_len, uint32_t frags_cap, uint32_t* open_off,
                       uint32_t* open_len, uint32_t opens_cap) {
    FrmArgs a{};
    a.blob = blob;
    a.cap = cap;
    a.off = off;
    a.nconn = nconn;
    a.conns = reinterpret_cast<uint4*>(conns);
    a.conn_blk_off = conn_blk_off;
    a.conn_frag_off = conn_frag_off;
    a.conn_open_off = conn_open_off;
    a.blocks = reinterpret_cast<uint4*>(blocks);
    a.blocks_cap = blocks_cap;
    a.frag_off = frag_off;
    a.frag_len = frag_len;
    a.frags_cap = frags_cap;
    a.open_off = open_off;
    a.open_len = open_len;
    a.opens_cap = opens_cap;
    hipLaunchKernelGGL(hpk_frmemit, dim3((nconn + kFrmWg - 1u) / kFrmWg), dim3(kFrmWg), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}

int hpk_launch_frmboff(hpk_ctx* c, const uint32_t* dst_off, uint32_t nfrags, const hpk_fblock* blocks, uint32_t nblocks,
                       uint32_t* block_off) {
    hipLaunchKernelGGL(hpk_frmboff, dim3(nblocks / kFrmWg + 1u), dim3(kFrmWg), 0, c->stream, dst_off, nfrags,
                       reinterpret_cast<const uint4*>(blocks), nblocks, block_off, c->d_err);
    HIP_TRY(hipGetLastError());
    return HPK_E_OK;
}

extern "C" int hpk_test_frmscan_geometry(uint32_t* wg_conns) {
    if (!wg_conns) return HPK_E_INVAL;
    *wg_conns = kFrmWg;
    return HPK_E_OK;
}
