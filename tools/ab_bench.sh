# same-box bench A/B over builds: in-tree ("new") and each abx/libuva_*.so, interleaved twice
# (plain python bench.py --steps 30: the headline steps only); results go to $OUT_DIR (default bench_out/)
set -o pipefail
export TMPDIR=/tmp
O="${OUT_DIR:-bench_out}"
mkdir -p "$O"
for i in 1 2; do
  for L in new abx/libuva_*.so; do
    if [ $L = new ]; then PY=python; else PY="python tools/ab_run.py $L"; fi
    timeout -k 10 300 $PY bench.py --steps 30 > "$O/abb.json" 2>"$O/abb.err" || { tail -20 "$O/abb.err"; exit 1; }
    F="$O/abb.json" TAG="$L" python3 -c "
import json, os; d=json.load(open(os.environ['F'])); print(os.environ['TAG'], d['value'], d['ms_per_step_median'])"
  done
done
