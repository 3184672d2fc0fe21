#!/bin/bash
# Every benchmark line of the round on one box: bench.py --full (headline, c4) and
# bench_workloads.py (c3, c3 --logs, c3range, c5, c2e2e, txlog, commit, wire, ragged,
# document, values), then one JSON line per run in $O/all.jsonl
# (O = $BENCH_ALL_OUT, default bench_out/all).
set -o pipefail
cd "$GRAFT_REPO_ROOT" || exit 1
O="${BENCH_ALL_OUT:-bench_out/all}"
mkdir -p "$O"
timeout -k 10 300 python -u bench.py --full > "$O/c2.json" 2> "$O/c2.err" || exit 1
timeout -k 10 300 python -u bench.py --full --config c4 --no-cpu-baseline > "$O/c4.json" 2> "$O/c4.err" || exit 1
for w in c3 "c3 --logs" c3range c5 c2e2e txlog commit wire ragged document values; do
  tag=$(echo "$w" | tr -d ' -')
  timeout -k 10 300 python -u bench_workloads.py --workload $w > "$O/$tag.json" 2> "$O/$tag.err" || exit 1
done
for f in "$O"/*.json; do tail -n 1 "$f"; done > "$O/all.jsonl"
