set -e
cd "$(dirname "$0")/.."
OUT=${AGPT_OUT:-out}   # where the logs go (relative to the repository root)
mkdir -p $OUT
python tools/render.py --scene c5 --width 960 --height 540 --spp 32 --out $OUT/c5.png
python bench.py --full --workload c5 --steps 1 --warmup 1 --spp 16 --no-cpu-baseline > $OUT/bench_c5.log 2> $OUT/bench_c5.err || { tail -30 $OUT/bench_c5.err; exit 1; }
cat $OUT/bench_c5.log
