cd "$(dirname "$0")/.."
OUT=${HULC_PROFILE_OUT:-profile_out}        # output directory (kept out of git)
export TMPDIR=/tmp
mkdir -p $OUT/pa
rocprofv3 --kernel-trace --stats -d $OUT/pa -o k -- python3 bench.py --full --affordance --batch 32 --steps 5 --warmup 2 --no-cpu-baseline --no-graph > $OUT/pa.log 2>&1
python3 tools/rocpd_stats.py $(find $OUT/pa -name "*.db" | head -1) > $OUT/aff_stats.txt
rm -rf $OUT/pa
head -30 $OUT/aff_stats.txt | cut -c1-150
