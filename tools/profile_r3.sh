#!/bin/bash
# Round-3 profiles: rocprofv3 kernel stats and the two PMC passes (FETCH_SIZE, WRITE_SIZE: separate runs, no trace domain beside
# --pmc) of bench.py for the three carries on 25FV47, for the dense LP of config 3 with the block as double, and for the max-flow LP;
# then the full bench line (every BASELINE config) and the carry table.  Run on the GPU box from the repo root; the summaries
# land in gpurun_out/prof_r3 and are copied into profiles/ by hand.
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$R/gpurun_out/prof_r3
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
COMMON="--no-cpu-baseline --no-configs --no-concurrency-probe"
profile() {  # name, bench arguments
  local name=$1; shift
  rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats_$name -- python3 $R/bench.py --full --steps 3 --warmup 1 $COMMON "$@" > $OUT/bench_${name}_under_rocprof.json 2> $OUT/stats_$name.log
  find $OUT/stats_$name -name "*kernel_stats.csv" -exec cp {} $OUT/kernel_stats_$name.csv \;
  rm -rf $OUT/stats_$name
  rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/fetch_$name -- python3 $R/bench.py --full --steps 1 --warmup 0 $COMMON "$@" > /dev/null 2> $OUT/fetch_$name.log
  rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/write_$name -- python3 $R/bench.py --full --steps 1 --warmup 0 $COMMON "$@" > /dev/null 2> $OUT/write_$name.log
  python3 $R/tools/pmc_traffic.py $OUT/fetch_$name $OUT/write_$name $OUT/pmc_traffic_$name.json > $OUT/pmc_traffic_$name.txt 2>&1
  rm -rf $OUT/fetch_$name $OUT/write_$name
}
profile 25fv47 --carry 0
profile 25fv47_lu --carry 1
profile 25fv47_lui --carry 2
profile dense4096_f64 --workload dense4096 --dense-storage f64
profile maxflow --workload maxflow --crash 0
cd $R
python3 bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err
python3 tools/carry_table.py 25FV47 BNL1 GREENBEA 80BAU3B BNL2 CYCLE > $OUT/carry_table.txt 2>&1
ls -la $OUT
