cd "$(dirname "$0")/.."
OUT=${HULC_PROFILE_OUT:-profile_out}        # output directory (kept out of git)
export TMPDIR=/tmp
for d in 0 1 2; do
  mkdir -p $OUT/pp$d
  HULC_TAPS_DBG=$d rocprofv3 --kernel-trace --stats -d $OUT/pp$d -o k -- python3 bench.py --full --affordance --batch 32 --steps 3 --warmup 1 --no-cpu-baseline --no-graph > /dev/null 2>&1
  python3 tools/rocpd_stats.py $(find $OUT/pp$d -name "*.db" | head -1) | grep "wgrad_taps_kernel" | cut -c1-100
  rm -rf $OUT/pp$d
done
