#!/bin/bash
# Ablation builds of the 256 x 256 x 64 GEMM K loop (gemm_8wave.h, -DTRIBE_ABL_*): one GEMM-only library per variant under ab_tmp/
# (every GEMM unit compiled with the variant's flags; gemm_plan.o and abi.o as `make` left them)
# (git-ignored, travels with the gpurun snapshot).  scripts/gemm_ablation.py times them interleaved in one process.
#   base      the kernel as shipped            nolds    no fragment ds_reads (LDS-DMA + MFMA + barriers)
#   nostage   no LDS-DMA (reads + MFMA)        bare     neither (MFMA + barriers)          nomfma   LDS-DMA + reads, no MFMA
set -e
cd "$(dirname "$0")/../algonauts-2025_amd/csrc"
mkdir -p ../../ab_tmp
FL="-O3 -fPIC -std=c++17 --offload-arch=gfx950 -Wno-unused-function"
UNITS="gemm gemm_8wave_nb4 gemm_8wave_nb3 gemm_128 gemm_4wave"
build() {
  local objs="" pids="" u p
  for u in $UNITS; do /opt/rocm/bin/hipcc $FL $2 -c $u.hip -o ../../ab_tmp/${u}_abl_$1.o & pids="$pids $!"; objs="$objs ../../ab_tmp/${u}_abl_$1.o"; done
  for p in $pids; do wait $p; done
  /opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 $objs gemm_plan.o abi.o -o ../../ab_tmp/libgemm_abl_$1.so
}
build base ""
build nolds "-DTRIBE_ABL_NO_LDSREAD"
build nostage "-DTRIBE_ABL_NO_STAGE"
build bare "-DTRIBE_ABL_NO_LDSREAD -DTRIBE_ABL_NO_STAGE"
build nomfma "-DTRIBE_ABL_NO_MFMA"
build dmaonly "-DTRIBE_ABL_NO_MFMA -DTRIBE_ABL_NO_LDSREAD"
ls -la ../../ab_tmp/libgemm_abl_*.so
