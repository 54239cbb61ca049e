#!/bin/bash
# Mesh / sampling parity (incl. the batched sampler) and the configs[3] / configs[4] bench legs.
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export OUT=${OUT:-out}  # folder for this script's logs and profiles
mkdir -p "$OUT"
timeout -k 10 400 python -u -m pytest tests/test_gpu_mesh.py tests/test_gpu_e2e.py -m gpu -x -q --timeout 300 \
    --timeout-method thread > $OUT/t_obj.log 2>&1 || { tail -40 $OUT/t_obj.log; exit 1; }
tail -2 $OUT/t_obj.log
timeout -k 10 300 python bench.py --full --frames 8 --steps 1 --cpu-frames 0 --filter-frames 0 > $OUT/b_obj.log 2>&1 \
    || { tail -20 $OUT/b_obj.log; exit 1; }
python3 - <<'PY'
import json, os
OUT = os.environ["OUT"]
d = json.loads(open(OUT + "/b_obj.log").read().splitlines()[-1])
print("objects", d["objects"])
print("hybrid", d["hybrid_map"])
PY
