#!/bin/bash
# usage: collect_round.sh <tag>      (on the GPU box, from the repo root; output under ${PROFILE_OUT:-profile_out}/<tag>)
# Default bench line, rocprofv3 kernel stats of the same command, and the HBM-traffic passes.
tag=$1
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
out=${PROFILE_OUT:-profile_out}/$tag
mkdir -p $out
python bench.py --full > $out/bench_default.json 2> $out/bench_default.err || exit 1
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/stats -- python bench.py --full --no-cpu-baseline > $out/bench_under_rocprof.json 2> $out/rocprof.err || exit 2
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 300 rocprofv3 --pmc $c --output-format csv -d $out/traffic_$c -- python profiles/traffic_probe.py fast > $out/traffic_$c.log 2>&1 || exit 3
done
python profiles/traffic_summary.py fast $out/traffic_FETCH_SIZE/*/*counter_collection.csv $out/traffic_WRITE_SIZE/*/*counter_collection.csv $out/pmc_traffic.json > $out/traffic_summary.txt
cat $out/bench_default.json
