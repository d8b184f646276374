# same-box A/B of the in-tree build against abx/libuva_base.so: focused tests ($FOCUS) on the new build,
# then kbench mode $KB and the plain bench (30 headline steps) on both builds; results go to $OUT_DIR (default bench_out/)
set -o pipefail
O="${OUT_DIR:-bench_out}"
mkdir -p "$O"
export TMPDIR=/tmp
if [ -n "$FOCUS" ]; then
  timeout -k 10 400 python -u -m pytest $FOCUS -x -q --timeout 120 --timeout-method thread > "$O/ab_t.log" 2>&1 || { echo TEST_FAIL; tail -30 "$O/ab_t.log"; exit 1; }
  tail -1 "$O/ab_t.log"
fi
for L in base new; do
  if [ $L = base ]; then PY="python tools/ab_run.py abx/libuva_base.so"; else PY=python; fi
  if [ -n "$KB" ]; then echo "== $L kbench $KB"; timeout -k 10 200 $PY tools/tools_kbench.py $KB 2>&1 | grep -v amdgpu.ids || exit 1; fi
  if [ -n "$PYB" ]; then echo "== $L $PYB"; timeout -k 10 200 $PY $PYB 2>&1 | grep -v amdgpu.ids || exit 1; fi
  [ -n "$NOBENCH" ] && continue
  timeout -k 10 300 $PY bench.py --steps 30 > "$O/ab_$L.json" 2>"$O/ab_$L.err" || { tail -20 "$O/ab_$L.err"; exit 1; }
  F="$O/ab_$L.json" TAG="$L" python3 -c "
import json, os; d=json.load(open(os.environ['F'])); print(os.environ['TAG'], d['value'], d['ms_per_step_median'])"
done
