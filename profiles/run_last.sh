#!/bin/bash
# usage: [OUT_DIR=<dir>] bash profiles/run_last.sh <tag>   (the sequence / reserve GPU tests, then the whole bench line, --full)
set -u
TAG=$1
OUT_DIR=${OUT_DIR:-results}
cd ${GRAFT_REPO_ROOT:-.}
mkdir -p "$OUT_DIR"
( timeout 100 python -m pytest tests/test_seq_gpu.py -q -p no:cacheprovider --timeout 90 --tb=short 2>&1 | tail -25 ) > "$OUT_DIR/${TAG}_seq_tests.log"
( timeout 150 python bench.py --full 2> "$OUT_DIR/${TAG}_bench.err" | grep '^{' | tail -1 ) > "$OUT_DIR/${TAG}_bench.json"
tail -3 "$OUT_DIR/${TAG}_seq_tests.log"
python -c "
import json; d=json.load(open('$OUT_DIR/${TAG}_bench.json')); print('value', d['value'], 'long_run', d['long_run'], 'traffic', d['roofline']['traffic'], 'frac', d['roofline']['frac'])"
