#!/bin/bash
# Registers / LDS / scratch of the kernels in csrc/strsim_kernels.hip (device-only compile, then the code object's metadata).
#   bash bench_support/kernel_resources.sh [name-filter-regex | group] [EXTRA flags]
# groups: nearest -- the kernels of strsim_nearest_device (its own and the best-match kernels it reuses)
#         partial -- the kernels of the partial ratio (strsim_partial.h), and below them the edit-distance kernels (k_dist_*: the
#                    distances and the OSA similarity) and the Indel kernels whose headers it includes (their figures must not move
#                    when strsim_partial.h changes)
#         token   -- the kernels of the token ratios (strsim_token.h), and below them the edit-distance / Indel / partial kernels
#                    whose headers it includes (their figures must not move when strsim_token.h changes)
#         wratio  -- the kernels of WRatio and the token compositions (strsim_wratio.h), and below them the token / partial / Indel /
#                    edit-distance kernels whose headers it includes (their figures must not move when strsim_wratio.h changes)
#         extract -- the kernel of strsim_extract_device and the nearest / best-match kernels it reuses
#         cdist   -- the kernels of strsim_cdist_device and the best-match kernels beside them (k_match_lane: the same sweep with a list)
#         join    -- the kernels of strsim_join_device, the pack and length-order kernels it reuses and k_extract_lane beside them (the
#                    same sweep with a list)
#         match_join -- the ten k_match_join_lane kernels of strsim_match_join_device, k_match_lane beside them (the same scoring with
#                    a list) and the join kernels around the sweep
#         cluster -- the kernels of strsim_components_device (strsim_cluster_device adds none: it runs the join's) and the join's
#                    scan kernels they reuse
#         qgram   -- the kernels of q-gram similarity (strsim_qgram.h), and below them the Indel / edit-distance kernels whose headers
#                    it includes (their figures must not move when strsim_qgram.h changes)
#         qgram_join -- the twelve k_qgram_join_lane kernels of strsim_qgram_join_device and k_qgram_join_first, k_qgram_lane and
#                    k_match_join_lane beside them (the same gram masks per pair; the same skeleton) and the join kernels around the sweep
#         damerau -- the kernels of the unrestricted Damerau-Levenshtein calls (strsim_damerau.h), and below them the edit-distance
#                    kernels whose header it includes (their figures must not move when strsim_damerau.h changes)
#         distance_join -- the six k_distance_join_lane kernels of strsim_distance_join_device and k_distance_join_finish, k_nearest_lane,
#                    k_dl_lane and k_match_join_lane beside them (the same cores; the same skeleton) and the join kernels around the sweep
#         common  -- the kernels of the Hamming / prefix / postfix / LCSseq calls (strsim_common.h), and below them the Indel and
#                    edit-distance kernels whose headers it includes (their figures must not move when strsim_common.h changes)
ROOT=$(cd "$(dirname "$0")/.." && pwd); OUT=${TMPDIR:-/tmp}/strsim_co; mkdir -p $OUT
case "$1" in
    common) FILTER='k_common_|k_indel_|k_dist_' ;;
    damerau) FILTER='k_dl_|k_dist_' ;;
    qgram) FILTER='k_qgram_|k_indel_|k_dist_' ;;
    wratio) FILTER='k_wratio_|k_take_|k_max_f64|k_token_|k_partial_|k_indel_|k_dist_' ;;
    token) FILTER='k_token_|k_partial_|k_indel_|k_dist_' ;;
    partial) FILTER='k_partial_|k_indel_|k_dist_' ;;
    extract) FILTER='k_extract_|k_nearest_hist|k_nearest_scan|k_nearest_scatter|k_match_pack|k_match_clear|k_match_fold|k_match_merge' ;;
    cdist) FILTER='k_cdist_|k_match_pack|k_match_lane' ;;
    join) FILTER='k_join_|k_extract_|k_nearest_hist|k_nearest_scan|k_nearest_scatter|k_match_pack' ;;
    match_join) FILTER='k_match_join_|k_match_lane|k_join_|k_nearest_hist|k_nearest_scan|k_nearest_scatter|k_match_pack' ;;
    qgram_join) FILTER='k_qgram_join_|k_qgram_lane|k_match_join_|k_join_|k_nearest_hist|k_nearest_scan|k_nearest_scatter|k_match_pack' ;;
    distance_join) FILTER='k_distance_join_|k_nearest_lane|k_nearest_scores|k_dl_lane|k_match_join_|k_join_|k_nearest_hist|k_nearest_scan|k_nearest_scatter|k_match_pack' ;;
    cluster) FILTER='k_components_|k_join_scan_' ;;
    nearest) FILTER='k_nearest_|k_match_pack|k_match_clear|k_match_fold|k_match_merge' ;;
    *) FILTER=${1:-.} ;;
esac
hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I$ROOT/include -I$ROOT/polars-strsim_amd/csrc $2 \
  --cuda-device-only -c -x hip $ROOT/polars-strsim_amd/csrc/strsim_kernels.hip -o $OUT/k.co 2>/dev/null || { echo "compile failed"; exit 1; }
/opt/rocm/lib/llvm/bin/clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$OUT/k.co --output=$OUT/k.elf
/opt/rocm/lib/llvm/bin/llvm-readelf --notes $OUT/k.elf > $OUT/notes.txt
python3 - "$OUT/notes.txt" "$FILTER" <<'PY'
import re, subprocess, sys
t = open(sys.argv[1]).read()
for e in re.split(r'\n\s+- \.agpr_count:', t)[1:]:
    g = lambda k: (re.search(r'\.' + k + r':\s+(\S+)', e) or [None, '?'])[1]
    n = subprocess.run(['c++filt', g('name')], capture_output=True, text=True).stdout.strip()
    if re.search(sys.argv[2], n):
        print('%-64s vgpr %4s sgpr %4s lds %6s scratch %5s spill %s' % (n[:64], g('vgpr_count'), g('sgpr_count'), g('group_segment_fixed_size'), g('private_segment_fixed_size'), g('vgpr_spill_count')))
PY
