# same-box bench A/B over one env var, printing the traced rows matching PAT: ENVVAR=.. VALS=".." PAT=".." bash tools/ab_rows.sh
# results go to $OUT_DIR (default bench_out/)
O="${OUT_DIR:-bench_out}"
mkdir -p "$O"
for v in $VALS; do
  env $ENVVAR=$v timeout -k 10 300 python bench.py --full --other-configs "" --no-cpu-baseline --steps 20 --trace-out "$O/rows_$v.json" > "$O/ab_$v.json" 2>"$O/ab_$v.err" || { echo BENCH_FAIL $v; tail -5 "$O/ab_$v.err"; exit 1; }
  F="$O/ab_$v.json" ROWS="$O/rows_$v.json" TAG="$ENVVAR=$v" PAT="$PAT" python3 -c "
import json, os, re; d=json.load(open(os.environ['F'])); print(os.environ['TAG'], d['value'], d['ms_per_step_median'])
for r in json.load(open(os.environ['ROWS'])):
    if re.search(os.environ['PAT'], r['kernel']): print('   %7.3f ms x%4.1f %6.0f TF  %s' % (r['avg_ms'], r['launches_per_step'], r['tflops'], r['kernel']))"
done
