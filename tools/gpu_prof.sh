set -e
cd "$(dirname "$0")/.."
OUT=${AGPT_OUT:-out}   # where the logs go (relative to the repository root)
mkdir -p $OUT/prof
export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o r01 -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline > $OUT/prof_bench.log 2> $OUT/prof_bench.err || { tail -30 $OUT/prof_bench.err; exit 1; }
cat $OUT/prof_bench.log | cut -c1-400
find $OUT/prof -name "*stats*" | head
f=$(find $OUT/prof -name "*kernel_stats.csv" | head -1)
cat $f | head -20
