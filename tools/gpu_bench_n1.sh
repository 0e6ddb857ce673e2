#!/bin/bash
# The N=1 bench command with every section (--full), timed; line in
# $OUT_DIR/bench_n1.json (default bench_out/), stderr in bench_n1.err; the
# full record is the detail file bench.py --full writes.
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
O=${OUT_DIR:-bench_out}
mkdir -p "$O"
t0=$(date +%s.%N)
timeout -k 10 600 python bench.py --full > "$O/bench_n1.json" 2> "$O/bench_n1.err" || exit 5
t1=$(date +%s.%N)
# stdout must be exactly one line, the JSON line (the driver's contract)
python3 -c "import json,sys; ls=open('$O/bench_n1.json').read().strip().splitlines(); assert len(ls) == 1, f'{len(ls)} stdout lines'; l=ls[0]; d=json.loads(l); print('line bytes', len(l), 'wall_s', round($t1-$t0,1), 'value', d['value'], 'frac', d['roofline']['frac'], 'cpu', d.get('cpu_baseline'))"
