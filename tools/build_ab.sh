#!/bin/bash
# variant library for A/B runs: tools/build_ab.sh <tag> "<extra hipcc flags>" [files]
#   -> rs-bann_amd/ab/librsbann_amd_<tag>.so
# files (default: every .hip source; the Makefile's SRCS is the list) are compiled with the flags;
# the other objects are taken from the in-tree build (make -C rs-bann_amd/csrc first)
# e.g. the fx gradient with its phase stamps: tools/build_ab.sh stamps "-DFX_STAMPS=1" kernels_fx
set -e
R=$(cd "$(dirname "$0")/.." && pwd); C=$R/rs-bann_amd/csrc
ALL=$(make -s --no-print-directory -C $C print-srcs)
TAG=$1; FLAGS=$2; FILES=${3:-$ALL}
O=/tmp/ab_$TAG; rm -rf $O; mkdir -p $O $R/rs-bann_amd/ab
for f in $FILES; do
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-result -munsafe-fp-atomics $FLAGS -c $C/$f.hip -o $O/$f.o 2>/dev/null &
done
wait
for f in $ALL; do
  [ -f $O/$f.o ] || cp $C/$f.o $O/$f.o
done
/opt/rocm/bin/hipcc -shared --offload-arch=gfx950 -o $R/rs-bann_amd/ab/librsbann_amd_$TAG.so $O/*.o $C/bann_net.o $C/bann_io.o -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
echo built $R/rs-bann_amd/ab/librsbann_amd_$TAG.so
