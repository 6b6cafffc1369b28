export OUT=${OUT:-out}; mkdir -p "$OUT"
cd $GRAFT_REPO_ROOT
python bench.py --suite ref --suite-out $OUT/r03_ref_suite.json > $OUT/r03_ref_suite.log 2> $OUT/r03_ref_suite.err
tail -1 $OUT/r03_ref_suite.log; tail -3 $OUT/r03_ref_suite.err
(time python bench.py --full > $OUT/r3_bench_default.json 2> $OUT/r3_bench_default.err) 2>&1 | grep real
python -c "
import json; d=json.load(open('$OUT/r3_bench_default.json')); print(d['ms_per_step'], d['cpu_baseline'].get('kernel_sets_tried'), d['roofline'].get('traffic'), d['roofline'].get('traffic_stale'), d['roofline'].get('frac_whole_factor'))"
python bench.py --full --gpus 2; echo "rc=$?"
