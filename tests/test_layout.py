"""The staging layouts of loona_amd/csrc/hpk_layout.h, run on the CPU (no GPU needed).

tests/emu/layout_emu.cpp includes the REAL hpk_layout.h and prints every layout for the argument tuples below. Each
is compared, offset by offset and in `bytes`, with the arithmetic the call code carried itself before the helper
(hpk_ctx.hip at commit cc195cc and, for the block decoder's batch area, hpk_hpack.cpp at commit 8b25017, restated in OLD
below with their line ranges): the layouts are byte for byte the same.
Independently of those formulas every layout must also be sound: each region on a 16-byte boundary, the regions in
order and disjoint and each at least its element size times the count its call moves, a staged input followed by 16
bytes of slack, and `bytes` at least 16 past the last region's end.
The tuples are the smallest that can go wrong (counts 1, 3, 4, 5; byte sizes 0, 1, 15, 16, 17; nent, ndecs, nf and
ns at 0 and 1; both forms of the string decode and of the page-locked area) and one with the largest counts the
callers admit, which a 32-bit intermediate would wrap.
The program is also built with -fsanitize=address,undefined and run stand-alone."""

import itertools
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

COUNTS = (1, 3, 4, 5)
SIZES = (0, 1, 15, 16, 17)
N_MAX, HI_MAX, NH_MAX, U32 = 0x7FFFFFFE, 0xFFFFFFDF, 0x1FFFFFFF, 0xFFFFFFFF  # (HI_MAX: HPK_MAX_OFFSET)


def up16(x):
    return (x + 15) & ~15


# What hpk_ctx.hip computed at cc195cc: (offsets by region name, bytes).
def old_strings(in_bytes, n, dcap):  # strings_host, lines 723-726 and 731
    at_ioff = up16(in_bytes + 16)
    at_ooff = at_ioff + up16(4 * (n + 1))
    at_len = at_ooff + up16(4 * (n + 1))
    at_pol = at_len + up16(4 * n)
    at_st = at_pol + up16(n)
    at_out = at_st + up16(n)
    return dict(**{"in": 0}, ioff=at_ioff, ooff=at_ooff, len=at_len, pol=at_pol, st=at_st, out=at_out), at_out + dcap + 16


def old_strdec(dev_in, n, dcap, mirror):  # strdec_host, lines 861-864, 868 and (the mirror form's d_end) 871
    at_off = up16(dev_in + 16)
    at_end = at_off + up16(4 * (n + 1))
    at_ooff = at_end + up16(4 * n)
    at_len = at_ooff + up16(4 * (n + 1))
    at_con = at_len + up16(4 * n)
    at_st = at_con + up16(4 * n)
    at_out = at_st + up16(n)
    end = at_off + 4 if mirror else at_end
    return dict(**{"in": 0}, off=at_off, end=end, ooff=at_ooff, len=at_len, con=at_con, st=at_st, out=at_out), at_out + dcap + 16


def old_blkscan(hi, nblocks, fcap, scap):  # blkscan_host, lines 968-973
    offs = up16(4 * (nblocks + 1))
    at_boff = up16(hi + 16)
    at_foff = at_boff + offs
    at_soff = at_foff + offs
    at_st = at_soff + offs
    at_fields = at_st + up16(nblocks)
    at_so = at_fields + 16 * fcap
    at_se = at_so + up16(4 * scap)
    return (dict(**{"in": 0}, boff=at_boff, foff=at_foff, soff=at_soff, st=at_st, fields=at_fields, so=at_so, se=at_se),
            at_se + up16(4 * scap) + 16)


def old_blkhead(hi, nblocks):  # hpk_blocks_device, lines 1241-1243 and 1248
    offs = up16(4 * (nblocks + 1))
    at_boff = up16(hi + 16)
    at_foff = at_boff + offs
    at_soff = at_foff + offs
    at_st = at_soff + offs
    return dict(**{"in": 0}, boff=at_boff, foff=at_foff, soff=at_soff, st=at_st), at_st + up16(nblocks) + 16


def old_blkout(nf, ns, dcap):  # hpk_blocks_device, lines 1268-1270, 1272 and (fields at 0) 1275
    sw = up16(4 * (ns + 1))
    at_so = 16 * nf
    at_se = at_so + sw
    at_oo = at_se + sw
    at_ol = at_oo + sw
    at_ss = at_ol + sw
    at_out = at_ss + up16(ns)
    return dict(fields=0, so=at_so, se=at_se, oo=at_oo, ol=at_ol, ss=at_ss, out=at_out), at_out + dcap + 16


def old_blkpin(nf, nblocks, ns, dcap, plan, nd, ne):  # hpk_blocks_device, lines 1284-1290 and (fields at 0) 1344
    offs, sw = up16(4 * (nblocks + 1)), up16(4 * (ns + 1))
    h_foff = 16 * nf
    h_oo = h_foff + offs
    h_ol = h_oo + sw
    h_ss = h_ol + sw
    h_out = h_ss + up16(ns)
    h_res = up16(h_out + dcap + 16)
    h_tabs = h_res + 16 * nblocks
    h_hdr = h_tabs + 32 * nd
    h_ent = h_hdr + 16 * nf
    return (dict(fields=0, foff=h_foff, oo=h_oo, ol=h_ol, ss=h_ss, out=h_out, res=h_res, tabs=h_tabs, hdr=h_hdr, ent=h_ent),
            h_ent + 16 * ne + 16 if plan else h_out + dcap + 16)


def old_blkapply(nd, nblocks, ne, nf):  # hpk_blocks_device, lines 1298-1301, (dec_blk_off at 0) 1303 and (the memset) 1307
    a_off, a_blk = up16(4 * (nd + 1)), up16(4 * nblocks)
    at_blk = a_off
    at_tabs = at_blk + a_blk
    at_ent = at_tabs + 32 * nd
    at_res = at_ent + 16 * ne
    at_hdr = at_res + 16 * nblocks
    return dict(doff=0, blk=at_blk, tabs=at_tabs, ent=at_ent, res=at_res, hdr=at_hdr, zeroed=16 * (nblocks + nf)), at_hdr + 16 * nf + 16


def old_plan(arena_cap, nh, nb, ne, nent, in_cap, out_cap):  # hpk_plan_device, lines 1153-1160, 1165 and (the arena at 0) 1173
    ni = 3 * nh
    at_foff = up16(arena_cap + 16)
    at_hoff = at_foff + up16(4 * (2 * nh + 1))
    at_eoff = at_hoff + up16(4 * (nb + 1))
    at_eblk = at_eoff + up16(4 * (ne + 1))
    at_flag = at_eblk + up16(4 * nb)
    at_tabs = at_flag + up16(ne)
    at_ent = at_tabs + up16(32 * ne)
    at_reps = at_ent + up16(16 * nent)
    at_ioff = at_reps + 16 * nh
    at_ilen = at_ioff + up16(4 * ni)
    at_ipol = at_ilen + up16(4 * ni)
    at_in = at_ipol + up16(ni)
    at_inoff = at_in + up16(in_cap + 16)
    at_ooff = at_inoff + up16(4 * (ni + 1))
    at_olen = at_ooff + up16(4 * (ni + 1))
    at_st = at_olen + up16(4 * ni)
    at_boff = at_st + up16(ni)
    at_out = at_boff + up16(4 * (nb + 1))
    return (dict(arena=0, foff=at_foff, hoff=at_hoff, eoff=at_eoff, eblk=at_eblk, flag=at_flag, tabs=at_tabs, ent=at_ent, reps=at_reps,
                 ioff=at_ioff, ilen=at_ilen, ipol=at_ipol, **{"in": at_in}, inoff=at_inoff, ooff=at_ooff, olen=at_olen, st=at_st,
                 boff=at_boff, out=at_out), at_out + out_cap + 16)


# What hpk_hpack.cpp computed at 8b25017 (hpk_hdec_decode_blocks, lines 1077-1087): out_len's region as wide as the
# offsets' (off_b), the n status bytes at the buffer's end.
def old_hdecbatch(tot, otot, n):
    in_b, dec_b, off_b = up16(tot + 16), up16(otot + 16), up16(4 * (n + 1))
    at_in_off = in_b + dec_b
    at_st = at_in_off + 3 * off_b
    return (dict(**{"in": 0}, dec=in_b, in_off=at_in_off, out_off=at_in_off + off_b, len=at_in_off + 2 * off_b, st=at_st),
            in_b + dec_b + 3 * off_b + n + 16)


OLD = dict(hdecbatch=old_hdecbatch, strings=old_strings, strdec=old_strdec, blkscan=old_blkscan, blkhead=old_blkhead, blkout=old_blkout, blkpin=old_blkpin,
           blkapply=old_blkapply, plan=old_plan)


# What each call moves through a region, from its copies and its kernels' arguments: [(region, element size, count)]
# in buffer order, and the staged inputs (16 bytes of slack behind their count of bytes).
def regions(what, a):
    if what == "strings":
        b, n, dcap = a
        return [("in", 1, b), ("ioff", 4, n + 1), ("ooff", 4, n + 1), ("len", 4, n), ("pol", 1, n), ("st", 1, n), ("out", 1, dcap)], ["in"]
    if what == "hdecbatch":  # (both blobs carry the slack: the decode's stores may run past a string's bound)
        tot, otot, n = a
        return [("in", 1, tot), ("dec", 1, otot), ("in_off", 4, n + 1), ("out_off", 4, n + 1), ("len", 4, n), ("st", 1, n)], ["in", "dec"]
    if what == "strdec":
        b, n, dcap, mirror = a
        r = [("in", 1, b), ("off", 4, n + 1 if mirror else n), ("end", 4, n), ("ooff", 4, n + 1), ("len", 4, n), ("con", 4, n), ("st", 1, n),
             ("out", 1, dcap)]
        return [x for x in r if not (mirror and x[0] == "end")], ["in"]  # (the mirror form's end lies inside off: its own test)
    if what in ("blkhead", "blkscan"):
        hi, nb = a[:2]
        r = [("in", 1, hi), ("boff", 4, nb + 1), ("foff", 4, nb + 1), ("soff", 4, nb + 1), ("st", 1, nb)]
        if what == "blkscan":
            r += [("fields", 16, a[2]), ("so", 4, a[3]), ("se", 4, a[3])]
        return r, ["in"]
    if what == "blkout":
        nf, ns, dcap = a
        return [("fields", 16, nf), ("so", 4, ns), ("se", 4, ns), ("oo", 4, ns + 1), ("ol", 4, ns), ("ss", 1, ns), ("out", 1, dcap)], []
    if what == "blkpin":
        nf, nb, ns, dcap, plan, nd, ne = a
        r = [("fields", 16, nf), ("foff", 4, nb + 1), ("oo", 4, ns + 1), ("ol", 4, ns), ("ss", 1, ns), ("out", 1, dcap)]
        if plan:
            r += [("res", 16, nb), ("tabs", 32, nd), ("hdr", 16, nf), ("ent", 16, ne)]
        return r, []
    if what == "blkapply":
        nd, nb, ne, nf = a
        return [("doff", 4, nd + 1), ("blk", 4, nb), ("tabs", 32, nd), ("ent", 16, ne), ("res", 16, nb), ("hdr", 16, nf)], []
    if what == "plan":
        cap, nh, nb, ne, nent, in_cap, out_cap = a
        ni = 3 * nh
        return [("arena", 1, cap), ("foff", 4, 2 * nh + 1), ("hoff", 4, nb + 1), ("eoff", 4, ne + 1), ("eblk", 4, nb), ("flag", 1, ne),
                ("tabs", 32, ne), ("ent", 16, nent), ("reps", 16, nh), ("ioff", 4, ni), ("ilen", 4, ni), ("ipol", 1, ni), ("in", 1, in_cap),
                ("inoff", 4, ni + 1), ("ooff", 4, ni + 1), ("olen", 4, ni), ("st", 1, ni), ("boff", 4, nb + 1), ("out", 1, out_cap)], ["arena", "in"]
    raise AssertionError(what)


def tuples():
    P = itertools.product
    t = [("strings", a) for a in P(SIZES, COUNTS, SIZES)]
    t += [("hdecbatch", a) for a in P(SIZES, SIZES, (0,) + COUNTS)]
    t += [("strdec", a) for a in P(SIZES, COUNTS, SIZES, (0, 1))]
    t += [("blkhead", a) for a in P(SIZES, COUNTS)]
    t += [("blkscan", a) for a in P(SIZES, COUNTS, (0, 1, 4, 5), (0, 1, 4, 5))]
    t += [("blkout", a) for a in P((0, 1, 3), (0, 1, 3, 4, 5), SIZES)]
    t += [("blkpin", a) for a in P((0, 1, 3), COUNTS, (0, 1, 4), (0, 1, 16, 17), (0, 1), (0, 1, 3), (0, 1, 5))]
    t += [("blkapply", a) for a in P((0, 1, 3, 4), COUNTS, (0, 1, 5), (0, 1, 3))]
    t += [("plan", a) for a in P(SIZES, COUNTS, (1, 3), (1, 4, 5), (0, 1), (0, 15, 17), (1, 16))]
    # the largest counts the callers admit
    t += [("hdecbatch", (U32, U32, U32)), ("strings", (HI_MAX, N_MAX, HI_MAX)), ("strdec", (HI_MAX, N_MAX, HI_MAX, 0)), ("strdec", (HI_MAX, N_MAX, HI_MAX, 1)),
          ("blkhead", (HI_MAX, N_MAX)), ("blkscan", (HI_MAX, N_MAX, U32, U32)), ("blkout", (U32, U32, U32)),
          ("blkpin", (U32, N_MAX, U32, U32, 0, 0, 0)), ("blkpin", (U32, N_MAX, U32, U32, 1, N_MAX, U32)),
          ("blkapply", (N_MAX, N_MAX, U32, U32)), ("plan", (HI_MAX, NH_MAX, N_MAX, N_MAX, U32, HI_MAX, HI_MAX))]
    return t


def _build(d, name, flags):
    exe = str(d / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", *flags, "-I", os.path.join(REPO, "loona_amd", "csrc"),
                           os.path.join(HERE, "emu", "layout_emu.cpp"), "-o", exe])
    return exe


def _run(exe, cases):
    text = "".join("%s %s\n" % (what, " ".join(str(x) for x in a)) for what, a in cases)
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr
    assert "ok: %d layouts" % len(cases) in p.stderr, p.stderr
    out = []
    for line in p.stdout.splitlines():
        what, *fields = line.split()
        got = {}
        for f in fields:
            k, v = f.split("=")
            got[k] = tuple(int(x) for x in v.split(":"))  # (offset, element size), or (value,)
        out.append((what, got))
    assert len(out) == len(cases)
    return p, out


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host C++ compiler")
    return tmp_path_factory.mktemp("layout_emu")


def check(cases, out):
    for (what, a), (name, got) in zip(cases, out):
        assert name == what
        tag = "%s%r" % (what, a)
        # the parent's formulas: every offset and the size
        want, want_bytes = OLD[what](*a)
        assert {k: v[0] for k, v in got.items() if k != "bytes"} == want, tag
        assert got["bytes"] == (want_bytes,), tag
        # and, whatever the formulas say, a sound layout
        regs, inputs = regions(what, a)
        assert [k for k in got if k in dict((r[0], 0) for r in regs)] == [r[0] for r in regs], tag  # printed in buffer order
        for i, (k, elem, count) in enumerate(regs):
            at, width = got[k]
            assert width == elem, (tag, k)
            assert at % 16 == 0, (tag, k)
            after = got[regs[i + 1][0]][0] if i + 1 < len(regs) else got["bytes"][0] - 16
            assert at + elem * count + (16 if k in inputs else 0) <= after, (tag, k)
        if what == "strdec" and a[3]:  # the mirror form: str_end is str_off + 1
            assert got["end"] == (got["off"][0] + 4, 4), tag
        if what == "blkapply":  # the results and the header records are zeroed in one piece
            assert got["hdr"][0] == got["res"][0] + 16 * a[1] and got["zeroed"] == (16 * (a[1] + a[3]),), tag


def test_layouts_equal_the_parents_and_are_sound(workdir):
    cases = tuples()
    assert len(cases) > 4000
    _, out = _run(_build(workdir, "layout_emu", []), cases)
    check(cases, out)


def test_layout_program_under_host_sanitizers(workdir):
    """The same program with ASan and UBSan, stand-alone, on the same tuples."""
    cases = tuples()
    exe = _build(workdir, "layout_emu_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    p, out = _run(exe, cases)
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr
    check(cases, out)
