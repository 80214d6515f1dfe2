#!/bin/bash
# A/B builds of the fast kernels: tools/build_variant.sh NAME -DPK_MIN_WAVES_FAST=5 ... -> parcels_amd/libparcels_hip_NAME.so
# (select it at run time with PARCELS_HIP_LIB=...; the other objects are those of the last `make`)
# Switches that select code: -DPK_FAST_LEAN=0 (pk_fast_agrid.h), -DPK_CG_LEAN=0 / -DPK_CG_NEAR=0 (pk_fast_cgrid.h); knobs: PK_MIN_WAVES_*, PK_CG_CACHE*
# (pk_kernels.h).  A change of the kernels themselves is compared against a build of the parent commit, selected the same way.
set -e
NAME=$1; shift
cd "$(dirname "$0")/../parcels_amd/csrc"
mkdir -p /tmp/pkv_$NAME
FL="-O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fPIC -Wall -Wno-unused-function"
for tu in ${PK_VARIANT_TUS:-pk_prog_rk4_fast pk_prog_rk4_fast_lp pk_prog_rk4_3d_fast}; do
  /opt/rocm/bin/hipcc $FL "$@" -c $tu.hip -o /tmp/pkv_$NAME/$tu.o &
done
wait
OBJS=""
for o in pk_api pk_api_sample pk_api_analysis pk_api_comm pk_host_stage pk_hashbuild pk_neighbors pk_interact pk_density pk_connectivity pk_random pk_unpack pk_prog_rk4 pk_prog_rk4_3d pk_prog_rk45 pk_prog_m1 pk_prog_generic pk_prog_typed pk_prog_rk4_fast pk_prog_rk4_fast_lp pk_prog_rk4_3d_fast pk_prog_cgrid_fast pk_prog_ux pk_prog_sigma pk_prog_eval_attached; do
  if [ -f /tmp/pkv_$NAME/$o.o ]; then OBJS="$OBJS /tmp/pkv_$NAME/$o.o"; else OBJS="$OBJS $o.o"; fi
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -pthread -o ../libparcels_hip_$NAME.so $OBJS
echo built ../libparcels_hip_$NAME.so
