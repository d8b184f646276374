# GPU round-trip: [focused tests] -> full -m gpu suite -> smoke -> bench --full (+ per-kernel trace rows)
# results go to $OUT_DIR (default bench_out/)
set -o pipefail
export TMPDIR=/tmp
O="${OUT_DIR:-bench_out}"
mkdir -p "$O"
if [ -n "$FOCUS" ]; then
  timeout -k 10 300 python -u -m pytest $FOCUS -x -v --timeout 120 --timeout-method thread > "$O/pytest_focus.log" 2>&1 || { echo FOCUS_FAIL; tail -40 "$O/pytest_focus.log"; exit 1; }
  tail -2 "$O/pytest_focus.log"
fi
if [ -n "$KB" ]; then
  timeout -k 10 200 python tools/tools_kbench.py $KB > "$O/kb.log" 2>&1 || { echo KB_FAIL; tail -20 "$O/kb.log"; exit 1; }
  cat "$O/kb.log"
fi
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > "$O/pytest_gpu.log" 2>&1 || { echo PYTEST_FAIL; tail -30 "$O/pytest_gpu.log"; exit 1; }
tail -2 "$O/pytest_gpu.log"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$O/smoke.log" 2>&1 || { echo SMOKE_FAIL; tail -30 "$O/smoke.log"; exit 1; }
tail -1 "$O/smoke.log"
timeout -k 10 600 python bench.py --full --trace-out "$O/trace_rows.json" > "$O/bench.json" 2> "$O/bench.err" || { echo BENCH_FAIL; tail -30 "$O/bench.err"; exit 1; }
cat "$O/bench.json"
