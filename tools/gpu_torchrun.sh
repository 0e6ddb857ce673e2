#!/bin/bash
# The multi-GPU bench command at N=2 and N=4 (ranks sharing one GPU):
# torchrun, every section of the line (--full). JSON in $OUT_DIR/tr_N.json
# (default bench_out/).
cd "$(dirname "$0")/.."
O=${OUT_DIR:-bench_out}
mkdir -p "$O"
P=29611
for n in ${NS:-2 4}; do
  P=$((P + 1))
  timeout -k 10 500 python -m torch.distributed.run --nnodes=1 --nproc-per-node $n --master-addr 127.0.0.1 \
    --master-port $P bench.py --full --gpus $n --steps 5 --warmup 2 > "$O/tr_$n.json" 2> "$O/tr_$n.err"
  rc=$?
  echo "N=$n rc=$rc"
  [ $rc -eq 0 ] || exit $rc
  python3 - "$O/tr_$n.json" <<'PY'
import json, sys
d = json.loads([l for l in open(sys.argv[1]) if l.startswith("{")][-1])
h = d["halo"]
pts = lambda k, c: [p[d[k]["cols"].index(c)] for p in d[k]["points"]]
print(d["value"], d["n_gpus"], h["us_per_iter"], h["rank0_phase_us"], d["halo_weak"]["us_per_iter"],
      pts("pingpong", "oneway_us"), pts("pingpong_1d", "oneway_us"), pts("alltoallv", "min_us"),
      pts("nbr_alltoallv", "min_us"), d.get("incomplete"), d["perf_model"].get("auto_model"))
PY
done
