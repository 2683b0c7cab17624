// hpk_layout.h — where each region of a staging buffer lies: one pure function per buffer that the host call
// layer carves (hpk_calls_*.hip). Host arithmetic only, no HIP header: tests/emu/layout_emu.cpp builds it with g++.
// Call code asks these for offsets and never adds staging sizes itself.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/hpk.h"

// A region's byte offset in its buffer, typed by its elements: the copy helpers (hpk_calls.h) take the width from it.
template <class T>
struct hpk_at {
    size_t at;
    T* in(void* base) const { return reinterpret_cast<T*>(static_cast<uint8_t*>(base) + at); }
};

// A bump allocator over byte offsets: every region starts on a 16-byte boundary.
struct hpk_carve {
    size_t end = 0;
    size_t take(size_t bytes) {
        const size_t at = end;
        end += (bytes + 15) & ~(size_t)15;
        return at;
    }
    template <class T>
    hpk_at<T> take(size_t count) { return {take(count * sizeof(T))}; }
    // a blob of `cap` bytes with 16 bytes of slack behind it (a call's input, staged at the buffer's start, keeps
    // its own absolute offsets there)
    hpk_at<uint8_t> blob(size_t cap) { return {take(cap + 16)}; }
};

// str_stage, the string-literal encode's host form: in | in_off | out_off | out_len | policy | status | out
struct hpk_lay_strings {
    hpk_at<uint8_t> in, pol, st, out;
    hpk_at<uint32_t> ioff, ooff, len;
    size_t bytes;
};
static inline hpk_lay_strings hpk_layout_strings(size_t in_bytes, size_t n, size_t dcap) {
    hpk_carve k;
    hpk_lay_strings l;
    l.in = k.blob(in_bytes);
    l.ioff = k.take<uint32_t>(n + 1);
    l.ooff = k.take<uint32_t>(n + 1);
    l.len = k.take<uint32_t>(n);
    l.pol = k.take<uint8_t>(n);
    l.st = k.take<uint8_t>(n);
    l.out = {k.end};
    l.bytes = k.end + dcap + 16;
    return l;
}

// sd_stage, the string-literal decode's host form: in | str_off | str_end | out_off | out_len | consumed | status |
// out. mirror (no str_end given): str_off has n + 1 entries and str_end is str_off + 1; its own region stays.
struct hpk_lay_strdec {
    hpk_at<uint8_t> in, st, out;
    hpk_at<uint32_t> off, end, ooff, len, con;
    size_t bytes;
};
static inline hpk_lay_strdec hpk_layout_strdec(size_t dev_in, size_t n, size_t dcap, bool mirror) {
    hpk_carve k;
    hpk_lay_strdec l;
    l.in = k.blob(dev_in);
    l.off = k.take<uint32_t>(n + 1);
    l.end = k.take<uint32_t>(n);
    if (mirror) l.end = {l.off.at + 4};
    l.ooff = k.take<uint32_t>(n + 1);
    l.len = k.take<uint32_t>(n);
    l.con = k.take<uint32_t>(n);
    l.st = k.take<uint8_t>(n);
    l.out = {k.end};
    l.bytes = k.end + dcap + 16;
    return l;
}

// The block decoder's Huffman batch (hpk_hdec.cpp), in the page-locked area: in | dec | in_off | out_off | out_len |
// status. Both blobs carry the 16 bytes of slack; out_len's region is as wide as the offsets' n + 1 entries, and the
// n status bytes end the buffer.
struct hpk_lay_hdecbatch {
    hpk_at<uint8_t> in, dec, st;
    hpk_at<uint32_t> in_off, out_off, len;
    size_t bytes;
    size_t in_cap() const { return dec.at - in.at; }  // the blobs' capacities, slack included
    size_t dec_cap() const { return in_off.at - dec.at; }
};
static inline hpk_lay_hdecbatch hpk_layout_hdecbatch(size_t tot, size_t otot, size_t n) {
    hpk_carve k;
    hpk_lay_hdecbatch l;
    l.in = k.blob(tot);
    l.dec = k.blob(otot);
    l.in_off = k.take<uint32_t>(n + 1);
    l.out_off = k.take<uint32_t>(n + 1);
    l.len = k.take<uint32_t>(n + 1);
    l.st = {k.end};
    l.bytes = k.end + n + 16;
    return l;
}

// bs_stage. The head, all that the block decoder's device-scan path keeps there: blocks | block_off | field_off |
// str_blk_off | status. The block scan's host form has its lists behind it: fields | str_off | str_end.
struct hpk_lay_blkhead {
    hpk_at<uint8_t> in, st;
    hpk_at<uint32_t> boff, foff, soff;
    size_t bytes;
};
struct hpk_lay_blkscan : hpk_lay_blkhead {
    hpk_at<hpk_field> fields;
    hpk_at<uint32_t> so, se;
};
static inline void hpk_layout_blkhead(hpk_carve& k, hpk_lay_blkhead& l, size_t hi, size_t nblocks) {
    l.in = k.blob(hi);
    l.boff = k.take<uint32_t>(nblocks + 1);
    l.foff = k.take<uint32_t>(nblocks + 1);
    l.soff = k.take<uint32_t>(nblocks + 1);
    l.st = k.take<uint8_t>(nblocks);
    l.bytes = k.end + 16;
}
static inline hpk_lay_blkhead hpk_layout_blkhead(size_t hi, size_t nblocks) {
    hpk_carve k;
    hpk_lay_blkhead l;
    hpk_layout_blkhead(k, l, hi, nblocks);
    return l;
}
static inline hpk_lay_blkscan hpk_layout_blkscan(size_t hi, size_t nblocks, size_t fcap, size_t scap) {
    hpk_carve k;
    hpk_lay_blkscan l;
    hpk_layout_blkhead(k, l, hi, nblocks);
    l.fields = k.take<hpk_field>(fcap);
    l.so = k.take<uint32_t>(scap);
    l.se = k.take<uint32_t>(scap);
    l.bytes = k.end + 16;
    return l;
}

// bs_out, the device-scan path's outputs: fields | str_off | str_end | out_off | out_len | status | out (each of
// the four string arrays as wide as out_off's ns + 1 entries)
struct hpk_lay_blkout {
    hpk_at<hpk_field> fields;
    hpk_at<uint32_t> so, se, oo, ol;
    hpk_at<uint8_t> ss, out;
    size_t bytes;
};
static inline hpk_lay_blkout hpk_layout_blkout(size_t nf, size_t ns, size_t dcap) {
    hpk_carve k;
    hpk_lay_blkout l;
    l.fields = k.take<hpk_field>(nf);
    l.so = k.take<uint32_t>(ns + 1);
    l.se = k.take<uint32_t>(ns + 1);
    l.oo = k.take<uint32_t>(ns + 1);
    l.ol = k.take<uint32_t>(ns + 1);
    l.ss = k.take<uint8_t>(ns);
    l.out = {k.end};
    l.bytes = k.end + dcap + 16;
    return l;
}

// The page-locked area the device-scan path reads back into: fields | field_off | out_off | out_len | status | out;
// with a plan, behind them: results | tabs | headers | the tables' entries.
struct hpk_lay_blkpin {
    hpk_at<hpk_field> fields;
    hpk_at<uint32_t> foff, oo, ol;
    hpk_at<uint8_t> ss, out;
    hpk_at<hpk_block_result> res;
    hpk_at<hpk_dtab> tabs;
    hpk_at<hpk_header> hdr, ent;
    size_t bytes;
};
static inline hpk_lay_blkpin hpk_layout_blkpin(size_t nf, size_t nblocks, size_t ns, size_t dcap, bool plan, size_t ndecs, size_t nent) {
    hpk_carve k;
    hpk_lay_blkpin l;
    l.fields = k.take<hpk_field>(nf);
    l.foff = k.take<uint32_t>(nblocks + 1);
    l.oo = k.take<uint32_t>(ns + 1);
    l.ol = k.take<uint32_t>(ns + 1);
    l.ss = k.take<uint8_t>(ns);
    l.out = k.blob(dcap);
    l.bytes = l.out.at + dcap + 16;
    l.res = k.take<hpk_block_result>(nblocks);
    l.tabs = k.take<hpk_dtab>(ndecs);
    l.hdr = k.take<hpk_header>(nf);
    l.ent = k.take<hpk_header>(nent);
    if (plan) l.bytes = k.end + 16;
    return l;
}

// ba_buf, the device-apply path: dec_blk_off | dec_blk | tabs | the tables' entries | results | headers
struct hpk_lay_blkapply {
    hpk_at<uint32_t> doff, blk;
    hpk_at<hpk_dtab> tabs;
    hpk_at<hpk_header> ent, hdr;
    hpk_at<hpk_block_result> res;
    size_t zeroed;  // the bytes from res on that the call zeroes: the results and the header records
    size_t bytes;
};
static inline hpk_lay_blkapply hpk_layout_blkapply(size_t ndecs, size_t nblocks, size_t nent, size_t nf) {
    hpk_carve k;
    hpk_lay_blkapply l;
    l.doff = k.take<uint32_t>(ndecs + 1);
    l.blk = k.take<uint32_t>(nblocks);
    l.tabs = k.take<hpk_dtab>(ndecs);
    l.ent = k.take<hpk_header>(nent);
    l.res = k.take<hpk_block_result>(nblocks);
    l.hdr = k.take<hpk_header>(nf);
    l.zeroed = k.end - l.res.at;
    l.bytes = k.end + 16;
    return l;
}

// bp_buf, the device-plan path (ni = 3 nh items): arena | field_off | hdr_off | enc_blk_off | enc_blk | enc_flags |
// tabs | the tables' entries | reps | item_off | item_len | item_policy | the gathered items | their offsets |
// out_off | out_len | status | block_off | out
struct hpk_lay_plan {
    hpk_at<uint8_t> arena, flag, ipol, in, st, out;
    hpk_at<uint32_t> foff, hoff, eoff, eblk, ioff, ilen, inoff, ooff, olen, boff;
    hpk_at<hpk_dtab> tabs;
    hpk_at<hpk_header> ent;
    hpk_at<hpk_hrep> reps;
    size_t bytes;
};
static inline hpk_lay_plan hpk_layout_plan(size_t arena_cap, size_t nh, size_t nblocks, size_t nencs, size_t nent, size_t in_cap,
                                           size_t out_cap) {
    const size_t ni = 3 * nh;
    hpk_carve k;
    hpk_lay_plan l;
    l.arena = k.blob(arena_cap);
    l.foff = k.take<uint32_t>(2 * nh + 1);
    l.hoff = k.take<uint32_t>(nblocks + 1);
    l.eoff = k.take<uint32_t>(nencs + 1);
    l.eblk = k.take<uint32_t>(nblocks);
    l.flag = k.take<uint8_t>(nencs);
    l.tabs = k.take<hpk_dtab>(nencs);
    l.ent = k.take<hpk_header>(nent);
    l.reps = k.take<hpk_hrep>(nh);
    l.ioff = k.take<uint32_t>(ni);
    l.ilen = k.take<uint32_t>(ni);
    l.ipol = k.take<uint8_t>(ni);
    l.in = k.blob(in_cap);
    l.inoff = k.take<uint32_t>(ni + 1);
    l.ooff = k.take<uint32_t>(ni + 1);
    l.olen = k.take<uint32_t>(ni);
    l.st = k.take<uint8_t>(ni);
    l.boff = k.take<uint32_t>(nblocks + 1);
    l.out = {k.end};
    l.bytes = k.end + out_cap + 16;
    return l;
}

// fs_stage. The head, all that hpk_h2_read_frames' device path keeps there: bytes (the carries behind the call's) |
// off | conns | conn_blk_off | conn_frag_off | conn_open_off. The frame scan's host form has its lists behind it:
// blocks | frag_off | frag_len | open_off | open_len.
struct hpk_lay_frmhead {
    hpk_at<uint8_t> in;
    hpk_at<uint32_t> off, cboff, cfoff, cooff;
    hpk_at<hpk_fconn> conns;
    size_t bytes;
};
struct hpk_lay_frmscan : hpk_lay_frmhead {
    hpk_at<hpk_fblock> blocks;
    hpk_at<uint32_t> fo, fl, oo, ol;
};
static inline void hpk_layout_frmhead(hpk_carve& k, hpk_lay_frmhead& l, size_t hi, size_t nconn) {
    l.in = k.blob(hi);
    l.off = k.take<uint32_t>(nconn + 1);
    l.conns = k.take<hpk_fconn>(nconn);
    l.cboff = k.take<uint32_t>(nconn + 1);
    l.cfoff = k.take<uint32_t>(nconn + 1);
    l.cooff = k.take<uint32_t>(nconn + 1);
    l.bytes = k.end + 16;
}
static inline hpk_lay_frmhead hpk_layout_frmhead(size_t hi, size_t nconn) {
    hpk_carve k;
    hpk_lay_frmhead l;
    hpk_layout_frmhead(k, l, hi, nconn);
    return l;
}
static inline hpk_lay_frmscan hpk_layout_frmscan(size_t hi, size_t nconn, size_t bcap, size_t fcap, size_t ocap) {
    hpk_carve k;
    hpk_lay_frmscan l;
    hpk_layout_frmhead(k, l, hi, nconn);
    l.blocks = k.take<hpk_fblock>(bcap);
    l.fo = k.take<uint32_t>(fcap);
    l.fl = k.take<uint32_t>(fcap);
    l.oo = k.take<uint32_t>(ocap);
    l.ol = k.take<uint32_t>(ocap);
    l.bytes = k.end + 16;
    return l;
}

// fs_out, the device path's lists and gathered blocks: blocks | frag_off | frag_len | open_off | open_len | the
// fragments' packed offsets | block_off | out
struct hpk_lay_frmout {
    hpk_at<hpk_fblock> blocks;
    hpk_at<uint32_t> fo, fl, oo, ol, doff, boff;
    hpk_at<uint8_t> out;
    size_t bytes;
};
static inline hpk_lay_frmout hpk_layout_frmout(size_t nb, size_t nf, size_t no, size_t out_cap) {
    hpk_carve k;
    hpk_lay_frmout l;
    l.blocks = k.take<hpk_fblock>(nb);
    l.fo = k.take<uint32_t>(nf);
    l.fl = k.take<uint32_t>(nf);
    l.oo = k.take<uint32_t>(no);
    l.ol = k.take<uint32_t>(no);
    l.doff = k.take<uint32_t>(nf + 1);
    l.boff = k.take<uint32_t>(nb + 1);
    l.out = {k.end};
    l.bytes = k.end + out_cap + 16;
    return l;
}

// fw_stage, the frame write's host form: blocks | block_off | stream_id | max_frame | wire_off | status | out
struct hpk_lay_frmwrite {
    hpk_at<uint8_t> in, st, out;
    hpk_at<uint32_t> boff, sid, mf, woff;
    size_t bytes;
};
static inline hpk_lay_frmwrite hpk_layout_frmwrite(size_t hi, size_t nblocks, size_t dcap) {
    hpk_carve k;
    hpk_lay_frmwrite l;
    l.in = k.blob(hi);
    l.boff = k.take<uint32_t>(nblocks + 1);
    l.sid = k.take<uint32_t>(nblocks);
    l.mf = k.take<uint32_t>(nblocks);
    l.woff = k.take<uint32_t>(nblocks + 1);
    l.st = k.take<uint8_t>(nblocks);
    l.out = {k.end};
    l.bytes = k.end + dcap + 16;
    return l;
}
