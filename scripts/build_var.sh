#!/bin/bash
# Build a variant of the product library with extra preprocessor flags (experiments only):
#   scripts/build_var.sh NAME "-DHPK_SPREAD=0 ..."  ->  loona_amd/libhpk_NAME.so (select with HPK_LIB)
# Every device unit of the Makefile's DEV list is compiled with the flags (a library without one of them does not load).
set -e
cd "$(dirname "$0")/../loona_amd/csrc"
NAME=$1; FLAGS=$2
T=/tmp/hpkvar_$NAME; mkdir -p $T
H="/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -Wall -Wno-unused-function"
UNITS=$(sed -n 's/^DEV := //p' Makefile | sed 's/\.o//g')
OBJS=
for u in $UNITS; do
  $H $FLAGS -x hip --offload-arch=gfx950 -c -o $T/$u.o $u.hip &
  OBJS="$OBJS $T/$u.o"
done
wait
for u in $UNITS; do [ -s $T/$u.o ] || { echo "$u failed"; exit 1; }; done
HOST=$(sed -n 's/^HOST := //p' Makefile)
make -s $HOST
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o ../libhpk_$NAME.so $HOST $OBJS
echo built loona_amd/libhpk_$NAME.so
