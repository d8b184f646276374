# same-box bench A/B over one environment variable: ENVVAR=<name> VALS="a b ..." bash tools/ab_env.sh
# results go to $OUT_DIR (default bench_out/)
export O="${OUT_DIR:-bench_out}"
mkdir -p "$O"
for v in $VALS; do
  env $ENVVAR=$v timeout -k 10 300 python bench.py --full --other-configs "" --no-cpu-baseline > "$O/ab_$v.json" 2>"$O/ab_$v.err" || { echo BENCH_FAIL $v; tail -5 "$O/ab_$v.err"; exit 1; }
  F="$O/ab_$v.json" TAG="$ENVVAR=$v" python3 -c "
import json, os; d=json.load(open(os.environ['F'])); print(os.environ['TAG'], d['value'], d['ms_per_step_median'], [(k['kernel'][:34], k['avg_ms']) for k in d['top_kernels'][:6]])"
done
