// layout_emu.cpp — prints the staging layouts of the REAL hpk_layout.h for the argument tuples on its standard input,
// one per line: "<layout> <arguments as the layout function takes them>". For each it answers one line:
// "<layout> <region>=<offset>:<element size> ... bytes=<bytes>", the regions in the order the buffer holds them.
// tests/test_layout.py compares them with the formulas the call code had before the helper.
#include <stdio.h>
#include <string.h>

#include "hpk_layout.h"

template <class T>
static void put(const char* name, hpk_at<T> r) { printf(" %s=%zu:%zu", name, r.at, sizeof(T)); }
#define PUT(l, f) put(#f, (l).f)

int main() {
    char line[512], what[32];
    int lines = 0;
    while (fgets(line, sizeof line, stdin)) {
        unsigned long long a[7] = {0, 0, 0, 0, 0, 0, 0};
        const int got = sscanf(line, "%31s %llu %llu %llu %llu %llu %llu %llu", what, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6]);
        if (got < 1) continue;
        size_t bytes = 0;
        printf("%s", what);
        if (!strcmp(what, "strings") && got == 4) {
            const hpk_lay_strings l = hpk_layout_strings(a[0], a[1], a[2]);
            PUT(l, in), PUT(l, ioff), PUT(l, ooff), PUT(l, len), PUT(l, pol), PUT(l, st), PUT(l, out);
            bytes = l.bytes;
        } else if (!strcmp(what, "strdec") && got == 5) {
            const hpk_lay_strdec l = hpk_layout_strdec(a[0], a[1], a[2], a[3] != 0);
            PUT(l, in), PUT(l, off), PUT(l, end), PUT(l, ooff), PUT(l, len), PUT(l, con), PUT(l, st), PUT(l, out);
            bytes = l.bytes;
        } else if (!strcmp(what, "hdecbatch") && got == 4) {
            const hpk_lay_hdecbatch l = hpk_layout_hdecbatch(a[0], a[1], a[2]);
            PUT(l, in), PUT(l, dec), PUT(l, in_off), PUT(l, out_off), PUT(l, len), PUT(l, st);
            bytes = l.bytes;
        } else if (!strcmp(what, "blkhead") && got == 3) {
            const hpk_lay_blkhead l = hpk_layout_blkhead(a[0], a[1]);
            PUT(l, in), PUT(l, boff), PUT(l, foff), PUT(l, soff), PUT(l, st);
            bytes = l.bytes;
        } else if (!strcmp(what, "blkscan") && got == 5) {
            const hpk_lay_blkscan l = hpk_layout_blkscan(a[0], a[1], a[2], a[3]);
            PUT(l, in), PUT(l, boff), PUT(l, foff), PUT(l, soff), PUT(l, st), PUT(l, fields), PUT(l, so), PUT(l, se);
            bytes = l.bytes;
        } else if (!strcmp(what, "blkout") && got == 4) {
            const hpk_lay_blkout l = hpk_layout_blkout(a[0], a[1], a[2]);
            PUT(l, fields), PUT(l, so), PUT(l, se), PUT(l, oo), PUT(l, ol), PUT(l, ss), PUT(l, out);
            bytes = l.bytes;
        } else if (!strcmp(what, "blkpin") && got == 8) {
            const hpk_lay_blkpin l = hpk_layout_blkpin(a[0], a[1], a[2], a[3], a[4] != 0, a[5], a[6]);
            PUT(l, fields), PUT(l, foff), PUT(l, oo), PUT(l, ol), PUT(l, ss), PUT(l, out), PUT(l, res), PUT(l, tabs), PUT(l, hdr), PUT(l, ent);
            bytes = l.bytes;
        } else if (!strcmp(what, "blkapply") && got == 5) {
            const hpk_lay_blkapply l = hpk_layout_blkapply(a[0], a[1], a[2], a[3]);
            PUT(l, doff), PUT(l, blk), PUT(l, tabs), PUT(l, ent), PUT(l, res), PUT(l, hdr);
            printf(" zeroed=%zu", l.zeroed);
            bytes = l.bytes;
        } else if (!strcmp(what, "plan") && got == 8) {
            const hpk_lay_plan l = hpk_layout_plan(a[0], a[1], a[2], a[3], a[4], a[5], a[6]);
            PUT(l, arena), PUT(l, foff), PUT(l, hoff), PUT(l, eoff), PUT(l, eblk), PUT(l, flag), PUT(l, tabs), PUT(l, ent), PUT(l, reps);
            PUT(l, ioff), PUT(l, ilen), PUT(l, ipol), PUT(l, in), PUT(l, inoff), PUT(l, ooff), PUT(l, olen), PUT(l, st), PUT(l, boff);
            PUT(l, out);
            bytes = l.bytes;
        } else {
            printf(" ?\n");
            return 2;
        }
        printf(" bytes=%zu\n", bytes);
        ++lines;
    }
    fprintf(stderr, "ok: %d layouts\n", lines);
    return 0;
}
