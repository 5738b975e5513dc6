#!/bin/bash
# Round-5 evidence on the MI355X box (run through gpurun): bench lines (fp32 headline as the driver runs it, the 16-bit storage
# mode, the other BASELINE configs), rocprofv3 kernel statistics for both precisions, per-function step times, PMC traffic.
# Everything lands in gpurun_out/evidence/; the summaries to be judged are copied to profiles/r05_* by hand.
set -u
R=$GRAFT_REPO_ROOT; O=$R/gpurun_out/evidence; mkdir -p $O
cd $R
python bench.py --full --steps 20 --warmup 5 > $O/bench_fp32.json 2> $O/bench_fp32.err
python bench.py --full --steps 20 --warmup 5 --dtype fp16 > $O/bench_fp16.json 2>/dev/null
python bench.py --full --steps 10 --warmup 3 --dtype fp16 --plan half_norms=False > $O/bench_fp16_two_term_norms.json 2>/dev/null
python bench.py --full --steps 5 --warmup 2 --config guided_8x_256 --no-f32-run --no-cpu-baseline > $O/bench_guided_8x_256.json 2>/dev/null
python bench.py --full --steps 5 --warmup 2 --config independent_32x_512 --no-f32-run --no-cpu-baseline > $O/bench_independent_32x_512.json 2>/dev/null
python bench.py --full --steps 5 --warmup 2 --config independent_32x_512 --dtype fp16 > $O/bench_independent_32x_512_fp16.json 2>/dev/null
python bench.py --full --steps 8 --warmup 2 --no-graphs --no-f32-run --no-cpu-baseline > $O/bench_no_graphs.json 2>/dev/null
# what plan.branch_streams (parallel graph branches: off by default, HIP-runtime segfault) would buy, same box
python bench.py --full --steps 20 --warmup 5 --no-f32-run --no-cpu-baseline --plan branch_streams=True > $O/bench_branch_streams.json 2>/dev/null
python bench.py --full --steps 20 --warmup 5 --no-f32-run --no-cpu-baseline > $O/bench_fp32_again.json 2>/dev/null
python tools/step_functions.py > $O/step_functions.txt 2>&1
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d /tmp/prof -o ev -- python $R/bench.py --steps 5 --warmup 2 --no-cpu-baseline --no-f32-run > $O/bench_under_rocprof.json 2> /dev/null
python $R/tools/rocpd_summary.py /tmp/prof/ev_results.db > $O/kernel_stats.md
python $R/tools/rocpd_summary.py /tmp/prof/ev_results.db 400 > $O/kernel_stats_all.md
rocprofv3 --kernel-trace --stats -d /tmp/prof16 -o ev -- python $R/bench.py --dtype fp16 --steps 5 --warmup 2 > $O/bench_fp16_under_rocprof.json 2> /dev/null
python $R/tools/rocpd_summary.py /tmp/prof16/ev_results.db > $O/kernel_stats_fp16.md
for c in FETCH_SIZE WRITE_SIZE; do rocprofv3 --kernel-trace --pmc $c -d /tmp/pmc_$c -o p --output-format csv -- python $R/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-f32-run --no-graphs > /dev/null 2>&1; done
python $R/tools/pmc_traffic.py /tmp/pmc_FETCH_SIZE/*counter_collection.csv /tmp/pmc_WRITE_SIZE/*counter_collection.csv > $O/pmc_traffic.json
for c in FETCH_SIZE WRITE_SIZE; do rocprofv3 --kernel-trace --pmc $c -d /tmp/pmc16_$c -o p --output-format csv -- python $R/bench.py --dtype fp16 --steps 2 --warmup 1 --no-graphs > /dev/null 2>&1; done
python $R/tools/pmc_traffic.py /tmp/pmc16_FETCH_SIZE/*counter_collection.csv /tmp/pmc16_WRITE_SIZE/*counter_collection.csv > $O/pmc_traffic_fp16.json
cd $R
ls -la $O
