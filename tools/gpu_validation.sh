# One GPU-box session that produces everything profiles/ holds for a round: `bash tools/gpu_validation.sh <out dir>`
# (SKIP_TESTS=1 skips the test suite).  Order: tests, rocprofv3 kernel stats, the two PMC passes, then the full bench run,
# which reads the fresh profiles/pmc_traffic_C2.json for its `roofline.traffic`.
set -e
R=$GRAFT_REPO_ROOT
OUT=$(realpath -m "${1:?usage: bash tools/gpu_validation.sh <out dir>}")
mkdir -p $OUT && cd $R
if [ -z "$SKIP_TESTS" ]; then
timeout -k 10 600 python -m pytest tests -m gpu -x -q > $OUT/gpu_tests.log 2>&1 || { tail -30 $OUT/gpu_tests.log; exit 1; }
tail -3 $OUT/gpu_tests.log
fi
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats -o c2 -- python3 $R/bench.py > $OUT/stats.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_f -o f -- python3 $R/bench.py --steps 20 --warmup 5 > $OUT/pmc_f.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_w -o w -- python3 $R/bench.py --steps 20 --warmup 5 > $OUT/pmc_w.log 2>&1
cd $R
python tools/pmc_traffic.py $OUT/pmc_f $OUT/pmc_w $OUT/pmc_traffic_C2.json
cp $OUT/pmc_traffic_C2.json profiles/pmc_traffic_C2.json
find $OUT -name '*kernel_trace.csv' -delete; find $OUT -name '*.db' -delete
timeout -k 10 400 python bench.py --full --kernel-table $OUT/c2_table.json > $OUT/bench_c2.json 2> $OUT/bench_c2.err
tail -1 $OUT/bench_c2.json | cut -c1-300
du -sh $OUT
