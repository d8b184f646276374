#!/bin/bash
# Same-box A/B of an env switch on the plain bench run (headline steps only): bash tools/tools_ab.sh VAR "A B" [rounds]
# prints value per run, alternating A, B, A, B ... (box-to-box variance is ~2-5 %, larger than
# most single changes).  Two builds of the library: tools/ab_bench.sh.  Results go to $OUT_DIR (default bench_out/).
VAR=$1; VALS=$2; R=${3:-2}
O="${OUT_DIR:-bench_out}"
mkdir -p "$O"
for r in $(seq $R); do for v in $VALS; do
  tag=$(echo "$v" | tr '/.' '__')
  env $VAR=$v timeout -k 10 300 python3 bench.py --steps 10 --warmup 3 > "$O/ab_$tag.json" 2>/dev/null || exit 1
  F="$O/ab_$tag.json" TAG="$VAR=$v" python3 -c "import json,os; d=json.load(open(os.environ['F'])); print(os.environ['TAG'], d['value'], d['ms_per_step'])"
done; done
