#!/bin/bash
# Per-kernel times of the binned intersection at c3 (rocprofv3 --kernel-trace --stats around tools/gpu_isect_check.py benchone),
# one line per library. Runs on the GPU machine.
#   tools/gpu_isect_kernels.sh <tag> base <variant names...>   "base" = the default build; variant libraries of tools/mkvariant.sh
#                                                              (each with its libgsplat_amd_torch_<name>.so, set alongside)
TAG=$1; shift
R=${GRAFT_REPO_ROOT:-$PWD}; mkdir -p $R/gpurun_out/$TAG
cd /tmp && export TMPDIR=/tmp
for v in "$@"; do
  unset GSPLAT_AMD_LIB GSPLAT_AMD_TORCH_LIB
  if [ $v != base ]; then
    export GSPLAT_AMD_LIB=$R/gsplat_amd/csrc/libgsplat_amd_$v.so GSPLAT_AMD_TORCH_LIB=$R/gsplat_amd/csrc/libgsplat_amd_torch_$v.so; fi
  rocprofv3 --kernel-trace --stats --output-format csv -d $R/gpurun_out/$TAG/t$v -o t -- python $R/tools/gpu_isect_check.py benchone > $R/gpurun_out/$TAG/$v.log 2>&1
  echo "$v: $(find $R/gpurun_out/$TAG/t$v -name '*kernel_stats.csv' | head -1 | xargs grep 'gsx::bin_\|gsx::tile_plan' | sed 's/(gsx::BinArgs, unsigned int)/()/' | awk -F, '{n=$1; gsub(/"/,"",n); gsub(/\(.*/,"",n); gsub(/.*::/,"",n); printf "%s %.1f  ", n, $4/1000}')"
done
