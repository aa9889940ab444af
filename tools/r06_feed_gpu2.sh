#!/bin/bash
# round 6: device pixels as the Feeder's default - feeder tests, kernel times of a bs=64 batch, the fed c4 step
# usage: tools/r06_feed_gpu2.sh [output folder, default out]
set -x
cd "$(dirname "$0")/.."
O=${1:-out}; mkdir -p $O
timeout 1500 python -m pytest tests/test_feed_gpu.py tests/test_feeder_gpu.py -q -x 2>&1 | tail -15 > $O/r06_feed_gpu_tests2.txt
cat $O/r06_feed_gpu_tests2.txt
export TMPDIR=/tmp
rm -rf $O/feedprof
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/feedprof -- python tools/feeder_rate.py --workers 10 --backends thread --native 1 --pixels gpu --batches 16 > $O/r06_feed_prof_run.txt 2>&1
f=$(find $O/feedprof -name '*kernel_stats.csv' | head -1)
cp "$f" $O/r06_feed_kernel_stats.csv
head -8 $O/r06_feed_kernel_stats.csv
rm -rf $O/feedprof
timeout 900 python bench.py --full --workload c4 --steps 8 --warmup 2 > $O/r06_bench_c4_fed_gpu_pixels.json 2> $O/r06_bench_c4_fed_err.txt
cat $O/r06_bench_c4_fed_gpu_pixels.json
timeout 600 python bench.py --workload feeder --steps 16 --warmup 4 > $O/r06_bench_feeder.json 2>> $O/r06_bench_c4_fed_err.txt
cat $O/r06_bench_feeder.json
tail -5 $O/r06_bench_c4_fed_err.txt
