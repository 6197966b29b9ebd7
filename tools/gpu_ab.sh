# bench.py once per environment setting (A/B of run-time knobs and AGPT_LIB_VARIANT builds): bash tools/gpu_ab.sh "ENV=.." ...
# AB_ARGS: extra bench.py arguments (default: the C3 headline workload), AB_STEPS: timed steps (default 3)
set -e
cd "$(dirname "$0")/.."
OUT=${AGPT_OUT:-out}   # where the logs go (relative to the repository root)
mkdir -p $OUT
show() { python - "$1" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
r = d['roofline']
print("value %.1f Mrays/s (%.1f Msamples/s)  ms/step %.1f  trace %.1f (ext %.1f mis %.1f shadow %.1f)  non-trace %.1f  mean %s" % (
    d['value'], d['config']['msamples_per_s'], d['ms_per_step'], r['trace_ms_per_step'], r['trace_split_ms_per_step']['continuation'],
    r['trace_split_ms_per_step']['mis'], r['trace_split_ms_per_step']['shadow'], r["render_ms_per_step"] - r["trace_ms_per_step"], d["image_mean_rgb"]))
PY
}
for cfg in "$@"; do
  echo "== $cfg"
  env $cfg python bench.py --full --steps ${AB_STEPS:-3} --warmup 1 --no-cpu-baseline --no-secondary $AB_ARGS > $OUT/ab.log 2> $OUT/ab.err || { tail -20 $OUT/ab.err; exit 1; }
  show $OUT/ab.log
  grep "trace clock\|trace stats\|shade clock" $OUT/ab.err | cut -c1-400 || true
done
