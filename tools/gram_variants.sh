# Gram kernel duration (2M x 64 fp64, tools/gram_bench.py): the per-wave LDS-DMA ring kernel (gram_glds_kernel), its floors
# (PBN_GRAM_DEBUG 1 = no MFMAs, 2 = no DMA) and the float table (gram_glds_f32_kernel).
# Usage (GPU box): bash tools/gram_variants.sh
echo "== double table (gram_glds_kernel)"; bash tools/gram_timing.sh gram_v2 | grep "gram_glds\|per call"
# the floor variants exist in measurement builds only: rebuild the library with -DPBN_GRAM_MEASURE on the box, restore it afterwards
touch pybnesian_amd/csrc/stats_kernels.hip; make -C pybnesian_amd/csrc CXXFLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -DPBN_GRAM_MEASURE" > /dev/null
for d in 1 2; do echo "== PBN_GRAM_DEBUG=$d"; PBN_GRAM_DEBUG=$d bash tools/gram_timing.sh gram_v2d$d | grep "gram_glds\|per call"; done
touch pybnesian_amd/csrc/stats_kernels.hip; make -C pybnesian_amd/csrc > /dev/null
echo "== float table (gram_glds_f32_kernel)"; GRAM_DTYPE=f32 bash tools/gram_timing.sh gram_f32 | grep "gram_glds\|per call"
