# End-of-round evidence, all from the full bench command (run from the repo root):
#   the full bench line, kernel-trace + stats of `python bench.py --full`, a per-stream timeline, the PMC
#   passes (one counter group per run, kernel-trace only), bench lines of the other workloads.
export OUT=${OUT:-out}; mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
TAG=${1:-r02}
python bench.py --full > $OUT/${TAG}_bench_bal871.json 2> $OUT/${TAG}_bench.err
rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_stats -o s -- python bench.py --full --no-cpu-baseline > $OUT/${TAG}_stats_bench.json 2> $OUT/${TAG}_stats.err
python profiles/roofline_from_rocprof.py $OUT/${TAG}_stats $OUT/${TAG}_stats_bench.json ${TAG}_bench_bal871 > $OUT/${TAG}_roofline.txt 2>&1
cp profiles/${TAG}_bench_bal871_kernel_stats.txt profiles/rocprof_roofline.json $OUT/
python profiles/stream_timeline.py $OUT/${TAG}_stats > $OUT/${TAG}_bench_bal871_timeline.txt 2>&1
bash profiles/collect_pmc.sh
python profiles/make_pmc_traffic.py bal871 $OUT/pmc_d/d_results.db $OUT/pmc_e/e_results.db 2 "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of python bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-profile --no-extras (profiles/collect_pmc.sh), build ${TAG}" > $OUT/${TAG}_pmc_traffic.txt 2>&1
cp profiles/pmc_traffic.json $OUT/
for d in a b c d e f; do python profiles/summarize_pmc.py $OUT/pmc_$d/${d}_results.db; done > $OUT/${TAG}_bench_bal871_pmc.txt 2>&1
for w in tridiag grid82 flat50k bal-small; do python bench.py --full --workload $w --no-extras > $OUT/${TAG}_bench_$w.json 2>/dev/null; done
python bench.py --full > $OUT/${TAG}_bench_bal871_final.json 2>/dev/null
