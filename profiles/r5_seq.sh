# launch sequence (rocprofv3 kernel trace) of one factor(): bash profiles/r5_seq.sh TAG "bench args" [ENV=..]
export OUT=${OUT:-out}; mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
TAG=$1; ARGS=$2; shift; shift
rm -rf $OUT/${TAG}_stats
env "$@" timeout 300 rocprofv3 --kernel-trace -d $OUT/${TAG}_stats -o s -- python bench.py $ARGS --no-extras --no-cpu-baseline --no-profile --steps 2 --warmup 1 > $OUT/${TAG}.log 2>&1
python profiles/kseq.py $OUT/${TAG}_stats/s_results.db elimFactor > $OUT/${TAG}_seq.txt 2>&1
rm -rf $OUT/${TAG}_stats
tail -1 $OUT/${TAG}.log | cut -c1-200
