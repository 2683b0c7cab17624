#!/bin/bash
# Are the device kernels of two source trees the same code? Prints, per translation unit, the sha256 of its
# gfx950 device assembly with the compile-unit id lines taken out (they hash the file's path and time):
#   scripts/asm_same.sh <tree A> <tree B> [unit ...]       (default units: hpk_decode hpk_pack)
set -o pipefail
A=$1; B=$2; shift 2
units=${@:-hpk_decode hpk_pack}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
tmp=$(mktemp -d)
rc=0
for u in $units; do
  for t in A B; do
    dir=$([ $t = A ] && echo "$A" || echo "$B")
    $HIPCC -O3 -std=c++17 -x hip --offload-arch=gfx950 --cuda-device-only -S -o $tmp/$u.$t.s "$dir/loona_amd/csrc/$u.hip" 2>/dev/null || exit 2
    grep -v '__hip_cuid' $tmp/$u.$t.s | sha256sum | cut -c1-16 > $tmp/$u.$t.sum
  done
  a=$(cat $tmp/$u.A.sum); b=$(cat $tmp/$u.B.sum)
  echo "$u $a $b $([ $a = $b ] && echo same || echo DIFFERENT)"
  [ $a = $b ] || rc=1
done
rm -rf $tmp
exit $rc
