#!/bin/bash
# tools/build_variant.sh NAME [-DFLAG ...]: libvb2.so with the evaluation kernels (llk_kernels.hip, llk_passes.hip) compiled under extra flags -> build_variants/NAME/libvb2.so
# (same-box A/B through VB2_LIB_PATH; build_variants/ is git-ignored but travels with gpurun snapshots)
set -e
cd "$(dirname "$0")/../verifybamid_amd/csrc"
name=$1; shift
out=../../build_variants/$name
mkdir -p $out
# both units of the evaluation kernels, each under its own scheduler as in csrc/Makefile: without flags this is the shipping code
cc="/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-result"
$cc -mllvm -amdgpu-sched-strategy=iterative-ilp "$@" -c llk_kernels.hip -o $out/llk_kernels.o &
main_unit=$!
$cc "$@" -c llk_passes.hip -o $out/llk_passes.o
wait $main_unit
objs=$(ls *.o | grep -v 'llk_kernels\|llk_passes')
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $out/libvb2.so $out/llk_kernels.o $out/llk_passes.o $objs -lpthread -lz -ldl
echo built $out/libvb2.so
