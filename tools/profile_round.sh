cd "$(dirname "$0")/.."
OUT=${HULC_PROFILE_OUT:-profile_out}        # output directory (kept out of git)
export TMPDIR=/tmp
# per-kernel durations and counters are taken on ONE stream (the default two-stream encoders overlap launches: their traced durations would
# include each other's share of the chip); the default bench line at the end runs the shipped two-stream configuration
export HULC_ENC_STREAMS=0
export HULC_FORK=0            # (round 6: the forked branches overlap launches too; the default bench line below runs the shipped forked graph)
mkdir -p $OUT/pk $OUT/pf $OUT/pw $OUT/pm
rocprofv3 --kernel-trace --stats -d $OUT/pk -o k -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-secondary --no-graph > $OUT/pk.log 2>&1
rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/pf -o f -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-secondary --no-graph > $OUT/pf.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $OUT/pw -o w -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-secondary --no-graph > $OUT/pw.log 2>&1
# MFMA utilisation pass (north_star: "rocprof HBM GB/s and MFMA utilisation against chip peak"): SQ + GRBM counters only, own run
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_INSTS_VALU_MFMA_MOPS_BF16 SQ_BUSY_CYCLES GRBM_GUI_ACTIVE --kernel-trace -d $OUT/pm -o m -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-secondary --no-graph > $OUT/pm.log 2>&1
unset HULC_ENC_STREAMS HULC_FORK
python3 bench.py --full > $OUT/bench_default.log 2>&1
for d in pk pf pw; do f=$(find $OUT/$d -name "*.db" | head -1); echo $d $f; done
python3 tools/rocpd_stats.py $(find $OUT/pk -name "*.db" | head -1) > $OUT/k_stats.txt
python3 tools/rocpd_stats.py --pmc $(find $OUT/pf -name "*.db" | head -1) > $OUT/f_pmc.txt
python3 tools/rocpd_stats.py --pmc $(find $OUT/pw -name "*.db" | head -1) > $OUT/w_pmc.txt
python3 tools/rocpd_stats.py --mfma $(find $OUT/pm -name "*.db" | head -1) > $OUT/m_mfma.txt
rm -rf $OUT/pk $OUT/pf $OUT/pw $OUT/pm
tail -1 $OUT/bench_default.log | cut -c1-400
