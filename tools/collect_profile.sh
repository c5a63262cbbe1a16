#!/bin/bash
# Copy the summaries of one `tools/gpu.sh round TAG` run from its results directory ($ICP_OUT, default
# measurements/: scratch) into profiles/TAG (tracked).
# usage: bash tools/collect_profile.sh TAG
set -eu
TAG=$1
R=${ICP_OUT:-measurements}
D=profiles/$TAG
mkdir -p $D
cp $R/bench_$TAG.json $D/bench_1gpu.json
cp $R/prof_$TAG/bench_traced.json $D/bench_under_rocprof.json
cp $R/prof_$TAG/trace/*kernel_stats.csv $D/kernel_stats_bench.csv
cp $R/pytest_gpu_$TAG.log $D/pytest_gpu.log
python3 tools/pmc_traffic.py $R/prof_$TAG 10000000 1 > $D/traffic.json
cp $D/traffic.json profiles/traffic_latest.json
ls -la $D
