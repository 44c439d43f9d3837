#!/bin/bash
# bench line (`bench.py --full`) + `rocprofv3 --kernel-trace --stats` of the same bench command -> OUT/bench_line.json, OUT/bench_kernel_stats.csv
# usage: run_bench_prof.sh OUT   (used by refresh.sh)
set -u
O="$(mkdir -p "${1:?output directory}" && cd "$1" && pwd)"
R="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
cd "$R"
timeout 600 python bench.py --full > $O/bench_line.json 2> $O/bench_line.err
export TMPDIR=/tmp; cd /tmp; rm -rf /tmp/prof2
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof2 -o bench -- python $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-extras > $O/prof2.log 2>&1
F=$(find /tmp/prof2 -name "*kernel_stats.csv" | head -1)
if [ -n "$F" ]; then cp $F $O/bench_kernel_stats.csv; head -8 $F; else tail -5 $O/prof2.log; fi
tail -c 400 $O/bench_line.json
