#!/bin/bash
# Are the device kernels of two source trees the same code? Prints, per translation unit, the sha256 of its
# gfx950 device assembly with the compile-unit id lines taken out (they hash the file's path and time):
#   scripts/asm_same.sh [--by-kernel] <tree A> <tree B> [unit ...]       (default units: hpk_decode hpk_pack)
# DEFS goes to the compile (DEFS=-DHPK_DIAG: the diagnostic build's kernels).
# --by-kernel: one hash per kernel instead (its body from its label to its .Lfunc_end, its own symbol and the
# function index of its .LBB / .LJTI labels taken out), so that a kernel can be compared across a changed
# template signature and when other kernels of the unit come or go. Kernels of one template are paired in their
# order of appearance, equal bodies first (an instantiation may appear earlier in one tree); a line per kernel
# and tree, then same / DIFFERENT / only in A / only in B per pair.
# Exit status 1 if anything compared differs.
set -o pipefail
by_kernel=0
if [ "$1" = --by-kernel ]; then by_kernel=1; shift; fi
A=$1; B=$2; shift 2
units=${@:-hpk_decode hpk_pack}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
tmp=$(mktemp -d)
rc=0
for u in $units; do
  for t in A B; do
    dir=$([ $t = A ] && echo "$A" || echo "$B")
    $HIPCC -O3 -std=c++17 $DEFS -x hip --offload-arch=gfx950 --cuda-device-only -S -o $tmp/$u.$t.s "$dir/loona_amd/csrc/$u.hip" 2>/dev/null || exit 2
    grep -v '__hip_cuid' $tmp/$u.$t.s | sha256sum | cut -c1-16 > $tmp/$u.$t.sum
  done
  if [ $by_kernel = 1 ]; then
    python3 - $u $tmp/$u.A.s $tmp/$u.B.s <<'EOF' || rc=1
import hashlib, re, shutil, subprocess, sys

def kernels(path):  # [(symbol, hash, lines)] in order of appearance
    out, sym, body = [], None, []
    for line in open(path):
        m = re.match(r"(_Z\w+):", line)
        if sym is None and m:
            sym, body = m.group(1), []
        elif sym is not None and line.startswith(".Lfunc_end"):
            text = "".join(body).replace(sym[2:], "KERNEL")  # (its statics' names hold the symbol less its _Z)
            text = re.sub(r"(\.L|\b)(BB|JTI)\d+_", r"\1\2_", text)  # (the labels, and the comments that name them)
            text = re.sub(r"[ \t]+;", " ;", text)  # (a comment's column follows its label's length)
            out.append((sym, hashlib.sha256(text.encode()).hexdigest()[:16], len(body)))
            sym = None
        elif sym is not None:
            body.append(line)
    return out

def demangle(syms):
    if not syms or not shutil.which("c++filt"):
        return syms
    return subprocess.run(["c++filt"] + syms, capture_output=True, text=True, check=True).stdout.splitlines()

def template(sym):  # the mangled name less its template arguments and parameters
    parts, s = [], sym[3:] if sym.startswith("_ZN") else sym[2:]
    while (m := re.match(r"\d+", s)):
        n = int(m.group())
        parts.append(s[m.end():m.end() + n])
        s = s[m.end() + n:]
    return "::".join(parts) or sym

unit, ka, kb = sys.argv[1], kernels(sys.argv[2]), kernels(sys.argv[3])
names = dict(zip([k[0] for k in ka + kb], demangle([k[0] for k in ka + kb])))
bad = False
show = lambda t, k: print(f"{unit} {t} {k[1]} {k[2]:6d} {names[k[0]]}")
for tpl in dict.fromkeys(template(k[0]) for k in ka + kb):
    a, b = [k for k in ka if template(k[0]) == tpl], [k for k in kb if template(k[0]) == tpl]
    # equal bodies pair first, each with the first one of the other tree not yet taken (a kernel that other
    # kernels moved around is still itself); what is left pairs in order of appearance
    pairs, rest = [], list(b)
    for x in a:
        y = next((k for k in rest if k[1] == x[1]), None)
        if y: rest.remove(y)
        pairs.append([x, y])
    for p in pairs:
        if p[1] is None and rest: p[1] = rest.pop(0)
    for x, y in pairs + [[None, y] for y in rest]:
        if x: show("A", x)
        if y: show("B", y)
        print(f"{unit}   {'only in B' if not x else 'only in A' if not y else 'same' if x[1] == y[1] else 'DIFFERENT'}")
        bad |= bool(x and y and x[1] != y[1])
sys.exit(1 if bad else 0)
EOF
  else
    a=$(cat $tmp/$u.A.sum); b=$(cat $tmp/$u.B.sum)
    echo "$u $a $b $([ $a = $b ] && echo same || echo DIFFERENT)"
    [ $a = $b ] || rc=1
  fi
done
rm -rf $tmp
exit $rc
