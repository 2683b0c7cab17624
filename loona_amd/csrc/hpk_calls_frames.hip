// hpk_calls_frames.hip — the HTTP/2 frame entry points of the C ABI (include/hpk.h): the frame scan, the gather of
// its fragments into header blocks, the frame write, and the device paths of hpk_h2_read_frames and
// hpk_h2_write_headers (hpk_h2.cpp reaches them through the pointers that hpk_ctx_create installs).
#include <stdlib.h>

#include "hpk_calls.h"

// The frame scan's steps on device arrays (hpk_frmscan.hip has the list), s the stream's slot with fs_meta (12 bytes
// per connection) and pk_tmp (hpk_pack_tmp_bytes(nconn)) reserved: the count pass and the three scans. The emit pass
// is the caller's (hpk_h2_read_frames' path sizes its lists by the totals before it emits).
static int frmscan_counts(hpk_ctx* c, hpk_slot* s, const uint8_t* bytes, uint32_t cap, const uint32_t* off, uint32_t nconn,
                          const hpk_fconn* conns, uint32_t* conn_blk_off, uint32_t* conn_frag_off, uint32_t* conn_open_off) {
    uint32_t* nb = s->fs_meta.as<uint32_t>();
    uint32_t* nf = nb + nconn;
    uint32_t* no = nf + nconn;
    int rc;
    if ((rc = hpk_launch_frmcount(c, bytes, cap, off, nconn, conns, nb, nf, no)) ||
        (rc = hpk_len_scan(c, nb, nconn, conn_blk_off, s->pk_tmp.p)) || (rc = hpk_len_scan(c, nf, nconn, conn_frag_off, s->pk_tmp.p)))
        return rc;
    return hpk_len_scan(c, no, nconn, conn_open_off, s->pk_tmp.p);
}

static int frmscan_nospace(size_t nb, size_t blocks_cap, size_t nf, size_t frags_cap, size_t no, size_t opens_cap) {
    if (nb > blocks_cap) return hpk_set_err_msg("the block records pass blocks_cap", HPK_E_NOSPACE);
    if (nf > frags_cap) return hpk_set_err_msg("the closed fragments pass frags_cap", HPK_E_NOSPACE);
    if (no > opens_cap) return hpk_set_err_msg("the open fragments pass opens_cap", HPK_E_NOSPACE);
    return HPK_E_OK;
}

// The end of a scan call: a synchronous one reads the three totals back with the wait, then reports bad offsets
// (HPK_E_INVAL) before a list that did not fit (HPK_E_NOSPACE).
static int frmscan_end(hpk_ctx* c, const uint32_t* blk_n, size_t blocks_cap, const uint32_t* frag_n, size_t frags_cap,
                       const uint32_t* open_n, size_t opens_cap, int flags) {
    if (flags & HPK_ASYNC) return HPK_E_OK;
    uint32_t tot[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(&tot[0], blk_n, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&tot[1], frag_n, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&tot[2], open_n, 4, hipMemcpyDeviceToHost, c->stream));
    if (int rc = hpk_call_end(c, flags)) return rc;
    return frmscan_nospace(tot[0], blocks_cap, tot[1], frags_cap, tot[2], opens_cap);
}

// the host's check of the connections before anything is copied: hpkfrm::conn_ok's conditions
static int frm_check_conns(const uint32_t* off, uint32_t nconn, const hpk_fconn* conns, size_t cap) {
    if (hpk_check_offsets(off, nconn, cap)) return HPK_E_INVAL;
    for (uint32_t k = 0; k < nconn; ++k)
        if (conns[k].pending && ((size_t)conns[k].carry_off > cap || (size_t)conns[k].carry_len > cap - conns[k].carry_off))
            return hpk_set_err_msg("a pending connection's carry window passes the blob's capacity", HPK_E_INVAL);
    return HPK_E_OK;
}

// The host form: connections checked before anything is copied, the bytes staged in one piece (at their own offsets;
// the carry windows are only listed, so their bytes stay behind) into the slot's scratch beside the arrays, the steps,
// the three offset arrays and the states read back, then exactly the written records and windows.
static int frmscan_host(hpk_ctx* c, const uint8_t* bytes, size_t cap, const uint32_t* off, uint32_t nconn, hpk_fconn* conns,
                        hpk_fblock* blocks, size_t blocks_cap, uint32_t* conn_blk_off, uint32_t* frag_off, uint32_t* frag_len,
                        size_t frags_cap, uint32_t* conn_frag_off, uint32_t* open_off, uint32_t* open_len, size_t opens_cap,
                        uint32_t* conn_open_off) {
    if (frm_check_conns(off, nconn, conns, cap)) return HPK_E_INVAL;
    if (nconn == 0) {
        conn_blk_off[0] = conn_frag_off[0] = conn_open_off[0] = 0;
        return HPK_E_OK;
    }
    const uint32_t lo = off[0], hi = off[nconn];
    const size_t most_b = (hi - lo) / 9u, most_f = most_b + nconn;  // (a frame takes 9 octets or more; one carry a connection)
    const uint32_t bcap = (uint32_t)(blocks_cap < most_b ? blocks_cap : most_b);
    const uint32_t fcap = (uint32_t)(frags_cap < most_f ? frags_cap : most_f);
    const uint32_t ocap = (uint32_t)(opens_cap < most_f ? opens_cap : most_f);
    const hpk_lay_frmscan l = hpk_layout_frmscan(hi, nconn, bcap, fcap, ocap);
    hpk_slot* s;
    int rc;
    if ((rc = hpk_slot_acquire(c, &s)) ||
        (rc = hpk_slot_reserve(c, s, {{&s->fs_meta, 12 * (size_t)nconn}, {&s->pk_tmp, hpk_pack_tmp_bytes(nconn)}, {&s->fs_stage, l.bytes}})))
        return rc;
    const hpk_stage g{c->stream, s->fs_stage.as<uint8_t>()};
    HIP_TRY(g.up_range(l.in, bytes, lo, hi));
    HIP_TRY(g.up(l.off, off, (size_t)nconn + 1));
    HIP_TRY(g.up(l.conns, conns, nconn));
    // (the device's capacity check is against the caller's cap: a carry window may lie anywhere below it)
    if ((rc = frmscan_counts(c, s, g(l.in), (uint32_t)cap, g(l.off), nconn, g(l.conns), g(l.cboff), g(l.cfoff), g(l.cooff))) ||
        (rc = hpk_launch_frmemit(c, g(l.in), (uint32_t)cap, g(l.off), nconn, g(l.conns), g(l.cboff), g(l.cfoff), g(l.cooff), g(l.blocks),
                                 bcap, g(l.fo), g(l.fl), fcap, g(l.oo), g(l.ol), ocap)))
        return rc;
    HIP_TRY(g.back(conn_blk_off, l.cboff, (size_t)nconn + 1));
    HIP_TRY(g.back(conn_frag_off, l.cfoff, (size_t)nconn + 1));
    HIP_TRY(g.back(conn_open_off, l.cooff, (size_t)nconn + 1));
    HIP_TRY(g.back(conns, l.conns, nconn));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t nb = conn_blk_off[nconn], nf = conn_frag_off[nconn], no = conn_open_off[nconn];
    const size_t gb = nb < bcap ? nb : bcap, gf = nf < fcap ? nf : fcap, go = no < ocap ? no : ocap;
    HIP_TRY(g.back(blocks, l.blocks, gb));
    HIP_TRY(g.back(frag_off, l.fo, gf));
    HIP_TRY(g.back(frag_len, l.fl, gf));
    HIP_TRY(g.back(open_off, l.oo, go));
    HIP_TRY(g.back(open_len, l.ol, go));
    if (gb || gf || go) HIP_TRY(hipStreamSynchronize(c->stream));
    if ((rc = hpk_slot_commit(c, s)) || (rc = hpk_take_err(c))) return rc;
    return frmscan_nospace(nb, blocks_cap, nf, frags_cap, no, opens_cap);
}

// The frame scan (include/hpk.h).
extern "C" int hpk_scan_frames(hpk_ctx* c, const uint8_t* bytes, size_t cap, const uint32_t* off, uint32_t nconn, hpk_fconn* conns,
                               hpk_fblock* blocks, size_t blocks_cap, uint32_t* conn_blk_off, uint32_t* frag_off,
                               uint32_t* frag_len, size_t frags_cap, uint32_t* conn_frag_off, uint32_t* open_off,
                               uint32_t* open_len, size_t opens_cap, uint32_t* conn_open_off, int flags) {
    if (!c || !off || !conn_blk_off || !conn_frag_off || !conn_open_off || (nconn && !conns))
        return hpk_set_err_msg("null argument", HPK_E_INVAL);
    if (nconn >= 0x7FFFFFFFu / 3u) return hpk_set_err_msg("too many connections for the frame scan", HPK_E_INVAL);
    if (cap > HPK_MAX_OFFSET) return hpk_set_err_msg("the frame scan's blob passes HPK_MAX_OFFSET", HPK_E_INVAL);
    if (nconn && ((!bytes && cap) || (!blocks && blocks_cap) || ((!frag_off || !frag_len) && frags_cap) ||
                  ((!open_off || !open_len) && opens_cap)))
        return hpk_set_err_msg("null blob or list", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    if (!(flags & HPK_PTR_DEVICE))
        return frmscan_host(c, bytes, cap, off, nconn, conns, blocks, blocks_cap, conn_blk_off, frag_off, frag_len, frags_cap,
                            conn_frag_off, open_off, open_len, opens_cap, conn_open_off);
    if ((((uintptr_t)conns | (uintptr_t)blocks) & 15u) != 0) return hpk_set_err_msg("conns and blocks must be 16-byte aligned", HPK_E_INVAL);
    if (nconn == 0) {
        HIP_TRY(hipMemsetAsync(conn_blk_off, 0, 4, c->stream));
        HIP_TRY(hipMemsetAsync(conn_frag_off, 0, 4, c->stream));
        HIP_TRY(hipMemsetAsync(conn_open_off, 0, 4, c->stream));
        return frmscan_end(c, conn_blk_off, blocks_cap, conn_frag_off, frags_cap, conn_open_off, opens_cap, flags);
    }
    hpk_slot* s;
    int rc;
    if ((rc = hpk_slot_acquire(c, &s)) ||
        (rc = hpk_slot_reserve(c, s, {{&s->fs_meta, 12 * (size_t)nconn + 16}, {&s->pk_tmp, hpk_pack_tmp_bytes(nconn)}})))
        return rc;
    // (a blob or a list of no capacity: an address that exists for the kernels' base pointers; nothing of it is touched)
    if (!bytes || !cap) bytes = s->fs_meta.as<uint8_t>(), cap = 0;
    if (!blocks_cap) blocks = reinterpret_cast<hpk_fblock*>(s->fs_meta.p);
    if (!frags_cap) frag_off = frag_len = s->fs_meta.as<uint32_t>();
    if (!opens_cap) open_off = open_len = s->fs_meta.as<uint32_t>();
    if ((rc = frmscan_counts(c, s, bytes, (uint32_t)cap, off, nconn, conns, conn_blk_off, conn_frag_off, conn_open_off)) ||
        (rc = hpk_launch_frmemit(c, bytes, (uint32_t)cap, off, nconn, conns, conn_blk_off, conn_frag_off, conn_open_off, blocks,
                                 hpk_clamp_u32(blocks_cap), frag_off, frag_len, hpk_clamp_u32(frags_cap), open_off, open_len,
                                 hpk_clamp_u32(opens_cap))))
        return rc;
    if ((rc = hpk_slot_commit(c, s))) return rc;
    return frmscan_end(c, conn_blk_off + nconn, blocks_cap, conn_frag_off + nconn, frags_cap, conn_open_off + nconn, opens_cap, flags);
}

// The gather of the closed fragments into header blocks (include/hpk.h): the ordered pack, then the blocks' offsets.
extern "C" int hpk_frame_blocks(hpk_ctx* c, const uint8_t* bytes, size_t cap, const uint32_t* frag_off, const uint32_t* frag_len,
                                uint32_t nfrags, const hpk_fblock* blocks, uint32_t nblocks, uint8_t* out_blob, size_t out_cap,
                                uint32_t* block_off, int flags) {
    if (int rc = hpk_check_call(c, !block_off || (nfrags && (!frag_off || !frag_len)) || (nblocks && !blocks), flags, nfrags,
                                "frame gather", nullptr, nullptr))
        return rc;
    if (nblocks >= 0x7FFFFFFFu) return hpk_set_err_msg("too many blocks for the frame gather", HPK_E_INVAL);
    if (((uintptr_t)blocks & 15u) != 0) return hpk_set_err_msg("blocks must be 16-byte aligned", HPK_E_INVAL);
    if (nfrags && ((!bytes && cap) || (!out_blob && out_cap))) return hpk_set_err_msg("null blob", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    hpk_slot* s;
    int rc;
    if ((rc = hpk_slot_acquire(c, &s)) ||
        (rc = hpk_slot_reserve(c, s, {{&s->fs_out, 4 * ((size_t)nfrags + 1) + 16}, {&s->pk_tmp, hpk_pack_tmp_bytes(nfrags)}})))
        return rc;
    uint32_t* dst_off = s->fs_out.as<uint32_t>();
    if ((rc = hpk_pack_launch(c, bytes, hpk_clamp_cap(cap), frag_off, frag_len, nfrags, out_blob, hpk_clamp_cap(out_cap), dst_off,
                              s->pk_tmp.p, HPK_MAX_OFFSET)) ||
        (rc = hpk_launch_frmboff(c, dst_off, nfrags, blocks, nblocks, block_off)))
        return rc;
    if ((rc = hpk_slot_commit(c, s))) return rc;
    return hpk_packed_end(c, block_off + nblocks, out_cap, flags);
}

extern "C" int hpk_ctx_set_frame_scan(hpk_ctx* c, int kind) {
    if (!c || (kind != HPK_FRAME_SCAN_HOST && kind != HPK_FRAME_SCAN_DEVICE)) return hpk_set_err_msg("bad frame scan", HPK_E_INVAL);
    c->frame_scan = kind;
    return HPK_E_OK;
}

namespace {
// what hpk_frames_device hands over on success, freed on every other way out
struct FrmOut {
    hpk_fblock* blocks = nullptr;
    uint32_t *block_off = nullptr, *open_off = nullptr, *open_len = nullptr;
    uint8_t* blk = nullptr;
    bool keep = false;
    ~FrmOut() {
        if (keep) return;
        free(blocks);
        free(block_off);
        free(open_off);
        free(open_len);
        free(blk);
    }
};
template <class T>
bool frm_alloc(T** p, size_t count) {
    *p = static_cast<T*>(malloc((count ? count : 1) * sizeof(T)));
    return *p != nullptr;
}
}  // namespace

// hpk_h2_read_frames' device path (hpk_internal.h; HPK_FRAME_SCAN_DEVICE). The call's bytes go up once at their own
// offsets with the carries behind them (at off[nconn]), the offsets and the states beside them; the count pass and
// the scans run and the three totals come back (the first wait); the lists are sized by them; the emit pass, the
// ordered pack of the closed fragments and the blocks' offsets follow; the states, conn_open_off, the block records,
// block_off and the open windows come back (the second wait), and with block_off's last entry known, exactly the
// blocks' bytes (the third). The caller's states are written last, when nothing can fail any more.
int hpk_frames_device(hpk_ctx* c, hpk_frmjob* job) {
    if (!c || c->frame_scan != HPK_FRAME_SCAN_DEVICE) return HPK_FRAMES_NOT_SELECTED;
    if (!job) return HPK_E_OK;  // (the question alone)
    job->nblocks = 0;
    job->blocks = nullptr;
    job->block_off = job->open_off = job->open_len = nullptr;
    job->blk = nullptr;
    if (int rc = hpk_test_take_failure()) return rc;
    const uint32_t nconn = job->nconn;
    FrmOut o;
    if (nconn == 0) {
        if (!frm_alloc(&o.blocks, 0) || !frm_alloc(&o.block_off, 1) || !frm_alloc(&o.open_off, 0) || !frm_alloc(&o.open_len, 0) ||
            !frm_alloc(&o.blk, 0))
            return hpk_set_err_msg("out of memory", HPK_E_INVAL);
        o.block_off[0] = 0;
        job->conn_open_off[0] = 0;
    } else {
        if (nconn >= 0x7FFFFFFFu / 3u) return hpk_set_err_msg("too many connections for the frame scan", HPK_E_INVAL);
        const uint32_t lo = job->off[0], hi = job->off[nconn];
        const uint64_t cap = (uint64_t)hi + job->ncarry;
        if (cap > HPK_MAX_OFFSET) return hpk_set_err_msg("the call's bytes and the held fragments pass HPK_MAX_OFFSET", HPK_E_INVAL);
        HIP_TRY(hipSetDevice(c->device));
        const hpk_lay_frmhead lh = hpk_layout_frmhead(cap, nconn);
        hpk_slot* s;
        int rc;
        if ((rc = hpk_slot_acquire(c, &s)) ||
            (rc = hpk_slot_reserve(c, s, {{&s->fs_meta, 12 * (size_t)nconn}, {&s->pk_tmp, hpk_pack_tmp_bytes(nconn)}, {&s->fs_stage, lh.bytes}})))
            return rc;
        const hpk_stage g{c->stream, s->fs_stage.as<uint8_t>()};
        HIP_TRY(g.up_range(lh.in, job->bytes, lo, hi));
        if (job->ncarry) HIP_TRY(hipMemcpyAsync(g(lh.in) + hi, job->carry, job->ncarry, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(g.up(lh.off, job->off, (size_t)nconn + 1));
        HIP_TRY(g.up(lh.conns, job->conns, nconn));
        if ((rc = frmscan_counts(c, s, g(lh.in), (uint32_t)cap, g(lh.off), nconn, g(lh.conns), g(lh.cboff), g(lh.cfoff), g(lh.cooff))))
            return rc;
        uint32_t tot[3] = {0, 0, 0};
        HIP_TRY(hipMemcpyAsync(&tot[0], g(lh.cboff) + nconn, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(&tot[1], g(lh.cfoff) + nconn, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(&tot[2], g(lh.cooff) + nconn, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        const uint32_t nb = tot[0], nf = tot[1], no = tot[2];
        // the gathered blocks are fragments of the call's bytes and of the carries, each byte in at most one
        const uint32_t out_cap = (hi - lo) + job->ncarry;
        const hpk_lay_frmout lq = hpk_layout_frmout(nb, nf, no, out_cap);
        if ((rc = hpk_slot_reserve(c, s, {{&s->fs_out, lq.bytes}, {&s->pk_tmp, hpk_pack_tmp_bytes(nf) + 32}}))) return rc;
        const hpk_stage q{c->stream, s->fs_out.as<uint8_t>()};
        if ((rc = hpk_launch_frmemit(c, g(lh.in), (uint32_t)cap, g(lh.off), nconn, g(lh.conns), g(lh.cboff), g(lh.cfoff), g(lh.cooff),
                                     q(lq.blocks), nb, q(lq.fo), q(lq.fl), nf, q(lq.oo), q(lq.ol), no)) ||
            (rc = hpk_pack_launch(c, g(lh.in), (uint32_t)cap, q(lq.fo), q(lq.fl), nf, q(lq.out), out_cap, q(lq.doff), s->pk_tmp.p, out_cap)) ||
            (rc = hpk_launch_frmboff(c, q(lq.doff), nf, q(lq.blocks), nb, q(lq.boff))))
            return rc;
        hpk_fconn* st = nullptr;
        if (!frm_alloc(&st, nconn)) return hpk_set_err_msg("out of memory", HPK_E_INVAL);
        struct Free {
            void* p;
            ~Free() { free(p); }
        } free_st{st};
        if (!frm_alloc(&o.blocks, nb) || !frm_alloc(&o.block_off, (size_t)nb + 1) || !frm_alloc(&o.open_off, no) || !frm_alloc(&o.open_len, no))
            return hpk_set_err_msg("out of memory", HPK_E_INVAL);
        HIP_TRY(g.back(st, lh.conns, nconn));
        HIP_TRY(g.back(job->conn_open_off, lh.cooff, (size_t)nconn + 1));
        HIP_TRY(q.back(o.blocks, lq.blocks, nb));
        HIP_TRY(q.back(o.block_off, lq.boff, (size_t)nb + 1));
        HIP_TRY(q.back(o.open_off, lq.oo, no));
        HIP_TRY(q.back(o.open_len, lq.ol, no));
        HIP_TRY(hipStreamSynchronize(c->stream));
        const uint32_t total = o.block_off[nb];
        if (total > out_cap) return hpk_set_err_msg("the gathered blocks pass the call's bytes", HPK_E_DEVICE);
        if (!frm_alloc(&o.blk, total)) return hpk_set_err_msg("out of memory", HPK_E_INVAL);
        if (total) {
            HIP_TRY(q.back(o.blk, lq.out, total));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        if ((rc = hpk_slot_commit(c, s)) || (rc = hpk_take_err(c))) return rc;  // (a void connection: the caller's offsets are wrong)
        for (uint32_t k = 0; k < nconn; ++k) job->conns[k] = st[k];
        job->nblocks = nb;
    }
    o.keep = true;
    job->blocks = o.blocks;
    job->block_off = o.block_off;
    job->open_off = o.open_off;
    job->open_len = o.open_len;
    job->blk = o.blk;
    return HPK_E_OK;
}

// The frame write's host form: offsets and frame sizes checked before anything is copied, the blocks staged in one
// piece (at their own offsets) into the slot's scratch beside the arrays, the steps, wire_off and status read back
// with exactly min(wire_off[n], out_cap) octets (the total is known here: the host sums the same lengths).
static int frmwrite_host(hpk_ctx* c, const uint8_t* blocks, size_t cap, const uint32_t* block_off, uint32_t n, const uint32_t* stream_id,
                         const uint32_t* max_frame, uint8_t* out_blob, size_t out_cap, uint32_t* wire_off, uint8_t* status) {
    if (hpk_check_offsets(block_off, n, cap)) return HPK_E_INVAL;
    uint64_t total = 0;
    for (uint32_t b = 0; b < n; ++b) {
        if (!hpk_max_frame_ok(max_frame[b])) return hpk_set_err_msg("a max_frame of 0 or above 0xFFFFFF", HPK_E_INVAL);
        total += hpk_wire_len(block_off[b + 1] - block_off[b], max_frame[b]);
    }
    if (n == 0) {
        wire_off[0] = 0;
        return HPK_E_OK;
    }
    // (a total past HPK_MAX_OFFSET: the device voids every block and no octet comes back)
    const size_t get = total > HPK_MAX_OFFSET ? 0 : total < out_cap ? (size_t)total : out_cap;
    const uint32_t lo = block_off[0], hi = block_off[n];
    const hpk_lay_frmwrite l = hpk_layout_frmwrite(hi, n, get);
    const size_t tmp = hpk_pack_tmp_bytes(n);
    hpk_slot* s;
    int rc;
    if ((rc = hpk_slot_acquire(c, &s)) || (rc = hpk_slot_reserve(c, s, {{&s->fw_stage, l.bytes}, {&s->pk_tmp, tmp + 32}}))) return rc;
    const hpk_stage g{c->stream, s->fw_stage.as<uint8_t>()};
    HIP_TRY(g.up_range(l.in, blocks, lo, hi));
    HIP_TRY(g.up(l.boff, block_off, (size_t)n + 1));
    HIP_TRY(g.up(l.sid, stream_id, n));
    HIP_TRY(g.up(l.mf, max_frame, n));
    if ((rc = hpk_frmwrite_launch(c, g(l.in), hi, g(l.boff), n, g(l.sid), g(l.mf), g(l.out), (uint32_t)get, g(l.woff), g(l.st), s->pk_tmp.p)))
        return rc;
    HIP_TRY(g.back(wire_off, l.woff, (size_t)n + 1));
    HIP_TRY(g.back(status, l.st, n));
    HIP_TRY(g.back(out_blob, l.out, get));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if ((rc = hpk_slot_commit(c, s)) || (rc = hpk_take_err(c))) return rc;
    if (total > out_cap) return hpk_set_err_msg("the wire octets pass the output capacity", HPK_E_NOSPACE);
    return HPK_E_OK;
}

// The frame write (include/hpk.h).
extern "C" int hpk_write_frames(hpk_ctx* c, const uint8_t* blocks, size_t cap, const uint32_t* block_off, uint32_t nblocks,
                                const uint32_t* stream_id, const uint32_t* max_frame, uint8_t* out_blob, size_t out_cap,
                                uint32_t* wire_off, uint8_t* status, int flags) {
    if (!c || !block_off || !wire_off || (nblocks && (!stream_id || !max_frame || !status))) return hpk_set_err_msg("null argument", HPK_E_INVAL);
    if (nblocks >= 0x7FFFFFFFu) return hpk_set_err_msg("too many blocks for the frame write", HPK_E_INVAL);
    if (cap > HPK_MAX_OFFSET) return hpk_set_err_msg("the frame write's blob passes HPK_MAX_OFFSET", HPK_E_INVAL);
    if (nblocks && ((!blocks && cap) || (!out_blob && out_cap))) return hpk_set_err_msg("null blob", HPK_E_INVAL);
    HIP_TRY(hipSetDevice(c->device));
    if (!(flags & HPK_PTR_DEVICE)) return frmwrite_host(c, blocks, cap, block_off, nblocks, stream_id, max_frame, out_blob, out_cap, wire_off, status);
    if (nblocks == 0) return hpk_packed_empty(c, wire_off, out_cap, flags);
    const size_t tmp = hpk_pack_tmp_bytes(nblocks);
    hpk_slot* s;
    int rc;
    if ((rc = hpk_slot_acquire(c, &s)) || (rc = hpk_slot_reserve(c, s, {{&s->pk_tmp, tmp + 32}}))) return rc;
    hpk_in_or_codes(c, &blocks, &cap);
    hpk_out_or_tmp(s, tmp, &out_blob, &out_cap);
    if ((rc = hpk_frmwrite_launch(c, blocks, (uint32_t)cap, block_off, nblocks, stream_id, max_frame, out_blob, hpk_clamp_cap(out_cap), wire_off,
                                  status, s->pk_tmp.p)))
        return rc;
    if ((rc = hpk_slot_commit(c, s))) return rc;
    return hpk_packed_end(c, wire_off + nblocks, out_cap, flags);
}

extern "C" int hpk_ctx_set_frame_write(hpk_ctx* c, int kind) {
    if (!c || (kind != HPK_FRAME_WRITE_HOST && kind != HPK_FRAME_WRITE_DEVICE)) return hpk_set_err_msg("bad frame write", HPK_E_INVAL);
    c->frame_write = kind;
    return HPK_E_OK;
}

extern "C" uint64_t hpk_test_frame_write_calls(const hpk_ctx* c) { return c ? c->frame_write_calls : 0u; }

// hpk_h2_write_headers' device framing (hpk_internal.h; HPK_FRAME_WRITE_DEVICE): hpk_write_frames with host pointers.
int hpk_write_device(hpk_ctx* c, const uint8_t* blocks, size_t cap, const uint32_t* block_off, uint32_t nblocks,
                     const uint32_t* stream_id, const uint32_t* max_frame, uint8_t* out_blob, size_t out_cap, uint32_t* wire_off,
                     uint8_t* status) {
    if (!c || c->frame_write != HPK_FRAME_WRITE_DEVICE) return HPK_FRAMES_NOT_SELECTED;
    if (int rc = hpk_test_take_failure()) return rc;
    if (int rc = hpk_write_frames(c, blocks, cap, block_off, nblocks, stream_id, max_frame, out_blob, out_cap, wire_off, status, HPK_PTR_HOST))
        return rc;
    c->frame_write_calls += 1;
    return HPK_E_OK;
}
