cd "$(dirname "$0")/.."
OUT=${HULC_PROFILE_OUT:-profile_out}        # output directory (kept out of git)
export TMPDIR=/tmp
mkdir -p $OUT/prw
rocprofv3 --kernel-trace --stats -d $OUT/prw -o k -- python3 bench.py --full --real-world --steps 5 --warmup 2 --no-cpu-baseline --no-graph > $OUT/prw.log 2>&1
python3 tools/rocpd_stats.py $(find $OUT/prw -name "*.db" | head -1) > $OUT/rw_k_stats.txt
python3 bench.py --full --real-world --no-cpu-baseline > $OUT/bench_rw.log 2>&1
rm -rf $OUT/prw
tail -1 $OUT/bench_rw.log | cut -c1-300
head -30 $OUT/rw_k_stats.txt
