#!/bin/bash
# Radix sort parity, then every GPU test (the sort orders units, edges, voxels and grids), then the filter leg.
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export OUT=${OUT:-out}  # folder for this script's logs and profiles
mkdir -p "$OUT"
timeout -k 10 300 python -u -m pytest tests/test_gpu_sort.py -m gpu -x -q --timeout 200 --timeout-method thread \
    > $OUT/t_sort.log 2>&1 || { tail -40 $OUT/t_sort.log; exit 1; }
tail -1 $OUT/t_sort.log
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread \
    > $OUT/t_all.log 2>&1 || { tail -40 $OUT/t_all.log; exit 1; }
tail -1 $OUT/t_all.log
timeout -k 10 300 python bench.py --full --frames 8 --steps 1 --cpu-frames 0 > $OUT/b_sort.log 2>&1 \
    || { tail -20 $OUT/b_sort.log; exit 1; }
python3 -c "import json; d=json.loads(open('$OUT/b_sort.log').read().splitlines()[-1]); print('filtered', d['filtered']['ms_per_frame'], 'objects', d['objects']['ms'], 'hybrid', d['hybrid_map']['ms'])"
