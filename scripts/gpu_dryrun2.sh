#!/bin/bash
# dry run of the N = 2 control flow of bench.py on a ONE-GPU box (gloo, both ranks on cuda:0): does every rank reach every collective?
# usage: bash scripts/gpu_dryrun2.sh [out_dir]   (default: a fresh temporary directory; the script prints what it finds there)
REPO=${GRAFT_REPO_ROOT:-$(pwd)}; cd $REPO
OUT=${1:-$(mktemp -d)}; mkdir -p $OUT
export DMPNN_BENCH_BACKEND=gloo DMPNN_BENCH_DEVICE=0
timeout 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29517 bench.py --full --gpus 2 --steps 20 --warmup 5 > $OUT/out.json 2> $OUT/err.txt
echo "rc=$?"
python - "$OUT/out.json" <<'PY'
import json
import sys
t = open(sys.argv[1]).read().strip().splitlines()
print(len(t), "line(s)")
d = json.loads(t[-1])
print({k: d[k] for k in ("value", "n_gpus", "ms_per_step", "scaling")}, d.get("train_step"))
PY
tail -5 $OUT/err.txt | cut -c1-200
