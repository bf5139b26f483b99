#!/bin/bash
# Run on the GPU box: the measurements of profiles/r10_free_drift.md, this build against a previous build of the library.
# usage: scripts/free_drift_profile.sh <previous libcsi_hip.so> [out dir]
# Every step runs under its own time limit and the chain stops at the first failure.
set -o pipefail
BASE=$(realpath "$1"); OUT=${2:-results/r10_free_drift}
mkdir -p "$OUT"
date -u +"start %Y-%m-%dT%H:%M:%SZ" > "$OUT/clock.txt"
rocm-smi --showclocks >> "$OUT/clock.txt" 2>&1 || true
run() { echo "== $*" >&2; "$@"; }
# 1. headline, alternated: previous, this, previous, this, previous, this
for r in 1 2 3; do
  CSI_HIP_LIBRARY=$BASE run timeout -k 10 200 python bench.py --steps 10 --warmup 3 --no-cpu-baseline --no-full-step --no-unfused --no-structure > "$OUT/headline_prev_$r.json" 2> "$OUT/headline_prev_$r.err" &&
  run timeout -k 10 200 python bench.py --steps 10 --warmup 3 --no-cpu-baseline --no-full-step --no-unfused --no-structure > "$OUT/headline_this_$r.json" 2> "$OUT/headline_this_$r.err" || exit 1
done
# 2. OMIP-style 2048^2 sub-cycle: kind 1 on the previous build against kind 2 on this one (and kind 1 on this one), alternated; the
#    order inside a round is reversed in every other round (what runs first in a round must not look like a cost of its build)
for r in 1 2 3 4; do
  if [ $((r % 2)) = 1 ]; then
    CSI_HIP_LIBRARY=$BASE run timeout -k 10 200 python scripts/free_drift_profile.py subcycle 1 2048 5 >> "$OUT/omip_kind1_prev.jsonl" &&
    run timeout -k 10 200 python scripts/free_drift_profile.py subcycle 2 2048 5 >> "$OUT/omip_kind2_this.jsonl" &&
    run timeout -k 10 200 python scripts/free_drift_profile.py subcycle 1 2048 5 >> "$OUT/omip_kind1_this.jsonl" || exit 1
  else
    run timeout -k 10 200 python scripts/free_drift_profile.py subcycle 1 2048 5 >> "$OUT/omip_kind1_this.jsonl" &&
    run timeout -k 10 200 python scripts/free_drift_profile.py subcycle 2 2048 5 >> "$OUT/omip_kind2_this.jsonl" &&
    CSI_HIP_LIBRARY=$BASE run timeout -k 10 200 python scripts/free_drift_profile.py subcycle 1 2048 5 >> "$OUT/omip_kind1_prev.jsonl" || exit 1
  fi
done
#    ... and what the device ran in such a sub-cycle: a kernel trace of its own per configuration
for cfg in "1 prev" "2 this" "1 this"; do
  set -- $cfg
  if [ $2 = prev ]; then export CSI_HIP_LIBRARY=$BASE; else unset CSI_HIP_LIBRARY; fi
  run timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_omip_$1_$2" -o t -- python scripts/free_drift_profile.py subcycle $1 2048 5 > /dev/null 2> "$OUT/trace_omip_$1_$2.err" || exit 1
  f=$(find "$OUT/trace_omip_$1_$2" -name "*kernel_stats.csv" | head -1)
  [ -n "$f" ] && head -8 "$f" > "$OUT/omip_kernel_stats_kind$1_$2.csv"
done
unset CSI_HIP_LIBRARY
# 3. the free-drift dynamics launch, in a kernel trace of its own, beside k_free_drift at the same size; whole RK3 steps
for N in 2048 4096; do
  run timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_$N" -o t -- python scripts/free_drift_profile.py dynamics $N > "$OUT/dynamics_$N.json" 2> "$OUT/dynamics_$N.err" || exit 1
  f=$(find "$OUT/trace_$N" -name "*kernel_stats.csv" | head -1)
  [ -n "$f" ] && grep -E "Name|k_free_drift" "$f" > "$OUT/kernel_stats_$N.csv"
done
run timeout -k 10 300 python scripts/free_drift_profile.py rk3 2048 10 > "$OUT/rk3_2048.json" || exit 1
# 4. nothing existing moves: the named EVP cases, both builds, every array bit for bit
CSI_HIP_LIBRARY=$BASE run timeout -k 10 400 python scripts/compare_libs.py dump "$OUT/cmp_prev.npz" 24 > "$OUT/cmp_prev.log" 2>&1 &&
run timeout -k 10 400 python scripts/compare_libs.py dump "$OUT/cmp_this.npz" 24 > "$OUT/cmp_this.log" 2>&1 &&
run python scripts/compare_libs.py diff "$OUT/cmp_prev.npz" "$OUT/cmp_this.npz" | tee "$OUT/cmp_diff.txt" || exit 1
rm -f "$OUT/cmp_prev.npz" "$OUT/cmp_this.npz"
#    ... and the fields bench.py's last timed step leaves (u, v, sigma of the headline workload), both builds
CSI_HIP_LIBRARY=$BASE run timeout -k 10 200 python bench.py --steps 4 --warmup 2 --no-cpu-baseline --no-full-step --no-unfused --no-structure --dump-outputs "$OUT/dump_prev" > /dev/null 2> "$OUT/dump_prev.err" &&
run timeout -k 10 200 python bench.py --steps 4 --warmup 2 --no-cpu-baseline --no-full-step --no-unfused --no-structure --dump-outputs "$OUT/dump_this" > /dev/null 2> "$OUT/dump_this.err" || exit 1
for f in "$OUT"/dump_prev/*.npy; do cmp "$f" "$OUT/dump_this/$(basename "$f")" && echo "identical $(basename "$f")"; done | tee "$OUT/dump_diff.txt"
rm -rf "$OUT/dump_prev" "$OUT/dump_this"
# 5. the headline as `python bench.py` prints it (every secondary record included), once per build
CSI_HIP_LIBRARY=$BASE run timeout -k 10 400 python bench.py > "$OUT/plain_prev.json" 2> "$OUT/plain_prev.err" &&
run timeout -k 10 400 python bench.py > "$OUT/plain_this.json" 2> "$OUT/plain_this.err" || exit 1
rm -rf "$OUT"/trace_*
date -u +"end %Y-%m-%dT%H:%M:%SZ" >> "$OUT/clock.txt"
echo done
