#!/bin/bash
# MIOpen's solver search for every convolution shape of the bench workloads, kept as a user find-db (what MIOPEN_USER_DB_PATH points to);
# results and the db under $OUT (default out/)
set -e
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
out=${OUT:-out}
mkdir -p "$out/miopen_db"
export MIOPEN_USER_DB_PATH=$(cd "$out/miopen_db" && pwd)
t0=$(date +%s)
timeout -k 10 900 python3 bench.py --workload imagenet_free_at --steps 4 --warmup 1 --no-cpu-baseline > $out/finddb_fa.json 2> $out/finddb_fa.err
echo "free-AT with search: $(( $(date +%s) - t0 )) s"; grep -o '"value": [0-9.]*' $out/finddb_fa.json | head -1
timeout -k 10 300 python3 bench.py --steps 5 --warmup 2 --no-cpu-baseline --other-steps 3 --full > $out/finddb_default.json 2> $out/finddb_default.err
ls -la $out/miopen_db; du -sh $out/miopen_db
t0=$(date +%s)
timeout -k 10 600 python3 bench.py --workload imagenet_free_at --steps 4 --warmup 1 --no-cpu-baseline > $out/finddb_fa2.json 2> $out/finddb_fa2.err
echo "free-AT again, db present: $(( $(date +%s) - t0 )) s"; grep -o '"value": [0-9.]*' $out/finddb_fa2.json | head -1
