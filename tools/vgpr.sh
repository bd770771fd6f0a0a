#!/bin/bash
# VGPR / SGPR / scratch / spills of the kernels whose name matches a pattern (development aid; needs no GPU):
#   tools/vgpr.sh                                          the tier-1 kernels (t1_)
#   tools/vgpr.sh 'j2k_level|j2k_cols_fin|rows_inv'        the fused inverse levels and the last residual row passes
#   tools/vgpr.sh 'gather_chunks|group_ranges'             the chunk gather, the range of a device array and of many (array_stats.hip)
#   tools/vgpr.sh 'frame_errors'                           the per-frame error statistics of the audit (array_stats.hip)
#   tools/vgpr.sh 'time_fold'                              the fold of the reduce decode: statistics over time (array_stats.hip)
#   tools/vgpr.sh 'area_'                                  the two launches of the area series and its weight check (array_stats.hip)
#   tools/vgpr.sh 'regrid'                                 the two forms of the regrid decode's kernel (regrid.hip)
#   tools/vgpr.sh 'rank'                                   the count and the advance of the quantile decode's radix select (quantile.hip)
#   tools/vgpr.sh 'time_map'                               the two instances of the time-map decode's kernel (time_map.hip)
#   tools/vgpr.sh 'pair_fold'                              the three instances of the pair decode's kernel (pair_stats.hip)
#   tools/vgpr.sh 'spell_fold'                             the seven instances of the spell decode's kernel (spell_stats.hip)
#   tools/vgpr.sh 'time_fold|time_map|pair_fold|spell_fold'    every kernel whose body is the walk of time_walk.hpp
# Compiled with the Makefile's code-generation flags; run it at two commits to compare their register use.
pat="${1:-t1_}"
cd "$(dirname "$0")/../ebcc_amd/csrc"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
filt="$(dirname "$HIPCC")/../llvm/bin/llvm-cxxfilt"
[ -x "$filt" ] || filt=c++filt
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
for f in j2k_analysis j2k_rate residual_dwt array_stats regrid quantile time_map pair_stats spell_stats; do
  "$HIPCC" --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -fno-fast-math -I../../include -S --cuda-device-only -o "$tmp/$f.s" $f.hip 2>/dev/null
  awk '/\.name:/{n=$2} /\.vgpr_count:/{v=$2} /\.sgpr_count:/{s=$2} /\.private_segment_fixed_size:/{p=$2} /\.vgpr_spill_count:/{print n, v, s, p, $2}' "$tmp/$f.s" |
  while read -r n v s p sp; do
    d=$("$filt" "$n")
    [[ $d =~ k_[A-Za-z0-9_]+(\<[^\>]*\>)? ]] && d=${BASH_REMATCH[0]}
    [[ $d =~ $pat ]] && printf "%-32s vgpr %s sgpr %s scratch %s spill %s\n" "$d" "$v" "$s" "$p" "$sp"
  done
done
exit 0
