#!/bin/bash
# Spatial-sharding parity (tests/test_gpu_shard.py), then the N-rank rehearsal of bench.py's spatial leg.
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export OUT=${OUT:-out}  # folder for this script's logs and profiles
mkdir -p "$OUT"
timeout -k 10 300 python -u -m pytest tests/test_gpu_shard.py -m gpu -x -v --timeout 200 --timeout-method thread \
    > $OUT/t_shard.log 2>&1 || { tail -60 $OUT/t_shard.log; exit 1; }
grep -E "PASSED|FAILED|passed|failed" $OUT/t_shard.log | tail -8
bash tools/rehearse_ranks.sh 2 || { tail -30 $OUT/rehearse_2.log; exit 1; }
python3 - <<'PY'
import json, os
OUT = os.environ["OUT"]
d = json.loads([l for l in open(OUT + "/rehearse_2.log") if l.startswith("{")][-1])
print("value", d["value"], "spatial", d["spatial"])
PY
