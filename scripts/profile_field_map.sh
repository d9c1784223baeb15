#!/bin/bash
# Kernel times of the field map for profiles/ (DESIGN.md section 22), from the repo root: scripts/profile_field_map.sh [OUT.csv]
# Every case of scripts/field_map_bench.py in a run of its own under rocprofv3 --kernel-trace --stats (10 repetitions and
# the warm-up call: 11 launches), so that a row of the per-kernel summary is one case and not a mix of the cases that share
# a kernel instance.  Keeps the rows of the map and track kernels, the case's name in front.  The first failure ends it.
set -uo pipefail
csv=${1:-profiles/field_map_kernel_stats.csv}
tmp=$(mktemp -d)
export TMPDIR=/tmp
first=1
for c in reference_uniform_uv reference_bisquare_uv reference_uniform_all reference_uniform_uv_walk reference_bisquare_uv_walk \
         deformed_bisquare_uv_k4 deformed_bisquare_uv_k4_walk window512_uniform_uv track_points_512; do
  timeout -k 10 120 rocprofv3 --kernel-trace --stats --output-format csv -d "$tmp/$c" -o fm -- \
    python3 scripts/field_map_bench.py --reps 10 --only "$c" > "$tmp/$c.log" 2>&1 || { tail -5 "$tmp/$c.log"; echo "$c failed"; exit 1; }
  stats=$(find "$tmp/$c" -name '*kernel_stats.csv' | head -1)
  [ -n "$stats" ] || { echo "$c: no kernel summary"; exit 1; }
  if [ $first = 1 ]; then echo "\"Case\",$(head -1 "$stats")" > "$csv"; first=0; fi
  grep 'lk_field_map_kernel\|lk_track_kernel' "$stats" | sed "s/^/\"$c\",/" >> "$csv"
done
rm -rf "$tmp"
cat "$csv"
