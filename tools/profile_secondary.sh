# kernel stats of the two secondary configurations (BASELINE configs[3] and configs[4]) on the GPU box: eager runs under rocprofv3 + the default
# (hipGraph) bench lines.   usage: bash tools/profile_secondary.sh ; then HULC_ROUND=NN python tools/collect_secondary_profiles.py
cd "$(dirname "$0")/.."
OUT=${HULC_PROFILE_OUT:-profile_out}        # output directory (kept out of git)
export TMPDIR=/tmp
mkdir -p $OUT/pa $OUT/prw
rocprofv3 --kernel-trace --stats -d $OUT/pa -o k -- python3 bench.py --full --affordance --batch 32 --steps 5 --warmup 2 --no-cpu-baseline --no-graph > $OUT/pa.log 2>&1
python3 tools/rocpd_stats.py $(find $OUT/pa -name "*.db" | head -1) > $OUT/aff_stats.txt
rocprofv3 --kernel-trace --stats -d $OUT/prw -o k -- python3 bench.py --full --real-world --steps 5 --warmup 2 --no-cpu-baseline --no-graph > $OUT/prw.log 2>&1
python3 tools/rocpd_stats.py $(find $OUT/prw -name "*.db" | head -1) > $OUT/rw_stats.txt
rm -rf $OUT/pa $OUT/prw
python3 bench.py --full --affordance --no-cpu-baseline > $OUT/bench_aff_default.log 2>&1
python3 bench.py --full --real-world --no-cpu-baseline > $OUT/bench_rw_default.log 2>&1
head -8 $OUT/rw_stats.txt | cut -c1-150
