#!/bin/bash
# A second copy of the library that differs in the NTT's compile-time knobs only (csrc/ntt_plan.inc: HM_NTT_LOG_TILE, HM_NTT_THREADS,
# HM_NTT_DIRECT_LOG, HM_NTT_2PASS_MAX; ntt.hip: HM_NTT_TIMING_NO_ROUND_BARRIER).  The plan is read by the driver (ntt.hip) and by the C
# entries (capi_poly.hip), so both units are compiled with the knobs; the other objects are the tree's own:
#   tools/ab_ntt.sh p3 -DHM_NTT_2PASS_MAX=20   ->  gpurun_ab/libhalo2_mi355x_p3.so      (use: HALO2_MI355X_LIB=<path>, tools/ntt_plans.py)
set -e
tag=$1; shift
cd "$(dirname "$0")/../halo2-experiments_amd/csrc"
make -s libhalo2_mi355x.so
out=../../gpurun_ab; mkdir -p $out
for unit in ntt capi_poly; do
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-result "$@" -c $unit.hip -o $out/${unit}_$tag.o
done
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o $out/libhalo2_mi355x_$tag.so $out/ntt_$tag.o $out/capi_poly_$tag.o \
  $(make -s --no-print-directory print-objs | tr ' ' '\n' | grep -vx -e ntt.o -e capi_poly.o)
rm -f $out/ntt_$tag.o $out/capi_poly_$tag.o; ls -la $out/libhalo2_mi355x_$tag.so
