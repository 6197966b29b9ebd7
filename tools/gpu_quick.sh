# GPU parity suite + a short bench line + optional env A/B settings: bash tools/gpu_quick.sh ["ENV=.. ENV2=.." ...]
set -e
cd "$(dirname "$0")/.."
OUT=${AGPT_OUT:-out}   # where the logs go (relative to the repository root)
mkdir -p $OUT
python -m pytest tests -m gpu -x -q > $OUT/tests_q.log 2>&1 || { tail -40 $OUT/tests_q.log; exit 1; }
tail -2 $OUT/tests_q.log
show() { python - "$1" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
r = d['roofline']
print("value %.1f Mrays/s (queries %.1f, %.1f Msamples/s)  ms/step %.1f  trace %.1f (ext %.1f mis %.1f shadow %.1f)  non-trace %.1f" % (
    d['value'], d['config']['reference_queries_mrays_s'], d['config']['msamples_per_s'], d['ms_per_step'], r['trace_ms_per_step'],
    r['trace_split_ms_per_step']['continuation'], r['trace_split_ms_per_step']['mis'],
    r['trace_split_ms_per_step']['shadow'], r['render_ms_per_step'] - r['trace_ms_per_step']))
PY
}
python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-secondary > $OUT/bench_q.log 2> $OUT/bench_q.err || { tail -30 $OUT/bench_q.err; exit 1; }
show $OUT/bench_q.log
for cfg in "$@"; do
  echo "== $cfg"
  env $cfg python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-secondary > $OUT/ab.log 2> $OUT/ab.err || { tail -20 $OUT/ab.err; exit 1; }
  show $OUT/ab.log
  grep "trace clock\|trace stats" $OUT/ab.err | cut -c1-330 || true
done
