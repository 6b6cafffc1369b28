# round-5 evidence on the final sources (run through gpurun from the repo root): bash profiles/r5_final.sh
export OUT=${OUT:-out}; mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
timeout 1800 bash profiles/collect_round.sh r05
python profiles/kseq.py $OUT/r05_stats/s_results.db elimFactor > $OUT/r05_launch_sequence_bal871.txt 2>&1
timeout 900 bash profiles/r5_c4_profile.sh r05
timeout 600 bash profiles/r5_prof_solve.sh r05 pmc
timeout 300 bash profiles/r5_seq.sh r05_grid82 "--workload grid82"; cp $OUT/r05_grid82_seq.txt $OUT/r05_launch_sequence_grid82.txt
timeout 300 bash profiles/r5_seq.sh r05_grid8 "--workload grid82 --batch 8"; cp $OUT/r05_grid8_seq.txt $OUT/r05_launch_sequence_grid_batch8.txt
python bench.py --full --workload grid82 --batch 8 --no-extras --no-cpu-baseline 2>/dev/null | tail -1 > $OUT/r05_bench_grid82_batch8.json
python bench.py --full --workload grid82 --batch 64 --no-extras --no-cpu-baseline 2>/dev/null | tail -1 > $OUT/r05_bench_grid82_batch64.json
timeout 1500 python bench.py --suite ref --suite-out $OUT/r05_ref_suite.json > $OUT/r05_ref_suite.log 2>/dev/null; tail -1 $OUT/r05_ref_suite.log | cut -c1-300
rm -rf $OUT/*_stats $OUT/pmc_?
ls $OUT | grep r05
