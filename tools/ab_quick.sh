# focused GPU tests ($FOCUS) then the bench with its trace passes, without the extra configs / CPU baseline
# results go to $OUT_DIR (default bench_out/)
set -o pipefail
O="${OUT_DIR:-bench_out}"
mkdir -p "$O"
export TMPDIR=/tmp
timeout -k 10 400 python -u -m pytest $FOCUS -x -q --timeout 120 --timeout-method thread > "$O/quick_t.log" 2>&1 || { echo TEST_FAIL; tail -30 "$O/quick_t.log"; exit 1; }
tail -1 "$O/quick_t.log"
timeout -k 10 300 python bench.py --full --other-configs "" --no-cpu-baseline --steps 30 --trace-out "$O/quick_rows.json" > "$O/quick_b.json" 2>"$O/quick_b.err" || { tail -20 "$O/quick_b.err"; exit 1; }
F="$O/quick_b.json" python3 -c "
import json, os; d=json.load(open(os.environ['F'])); print(d['value'], d['ms_per_step_median'], [(k['kernel'][:40], k['avg_ms'], k['tflops']) for k in d['top_kernels'][:5]])"
