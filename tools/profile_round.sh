#!/bin/bash
# Produce the per-round profile artefacts on the GPU box; outputs under $OUT (default profile_out/).
export TMPDIR=/tmp
R=${1:-r01}
OUT=${OUT:-profile_out}
mkdir -p "$OUT"
python bench.py --full --steps 20 --warmup 5 > "$OUT"/bench_${R}.json 2> "$OUT"/bench_${R}.err
tail -c 400 "$OUT"/bench_${R}.json
rocprofv3 --kernel-trace --stats -d /tmp/prof_${R} -o trace -- python bench.py --steps 10 --warmup 3 --no-cpu-baseline --no-graph --no-train-mode --no-decode > "$OUT"/prof_${R}.log 2>&1
python tools/summarize_rocprof.py /tmp/prof_${R}/trace_results.db > "$OUT"/rocprof_${R}_kernel_stats.txt
head -30 "$OUT"/rocprof_${R}_kernel_stats.txt
