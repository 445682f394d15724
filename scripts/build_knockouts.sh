#!/bin/bash
# Experiment build: the knock-out switches of the dominant kernels (NSFEM_LATTICE_DBG, NSFEM_JL_DBG,
# NSFEM_SPMV_DEBUG -- parts of a kernel switched off, WRONG results) exist only in this variant.
# Output: build/knockouts/libnsfem_hip.so (never the product library); use it with
#   import _native as nat; nat.load_library("build/knockouts/libnsfem_hip.so")   (before any context is created)
set -e
cd "$(dirname "$0")/.."
SRC=navierstokes-with-fenics_amd/csrc
OUT=build/knockouts
mkdir -p $OUT
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -DNSFEM_KNOCKOUTS=1"
for f in assembly assembly3d boundary linalg multigrid comm api; do
  [ -f $SRC/$f.hip ] && /opt/rocm/bin/hipcc $FLAGS -c $SRC/$f.hip -o $OUT/$f.o &
done
/opt/rocm/bin/hipcc $FLAGS -x hip -c $SRC/pattern.cpp -o $OUT/pattern.o
wait
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o $OUT/libnsfem_hip.so $OUT/*.o -lrccl
echo "built $OUT/libnsfem_hip.so"
