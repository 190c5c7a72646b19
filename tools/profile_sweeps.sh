set -e
R=$GRAFT_REPO_ROOT
OUT=${PROFILE_OUT:-$R/profile_out}
cd /tmp && export TMPDIR=/tmp
for C in C4 C5; do
  rm -rf $OUT/ks_$C; mkdir -p $OUT/ks_$C
  timeout -k 10 280 rocprofv3 --kernel-trace --stats -d $OUT/ks_$C -o ks --output-format csv -- python3 $R/bench.py --config $C --only --steps 5 --warmup 2 --full --no-cpu-baseline > $OUT/ks_$C/run.log 2>&1
  for K in FETCH_SIZE WRITE_SIZE; do
    rm -rf $OUT/pmc/${C}_$K; mkdir -p $OUT/pmc/${C}_$K
    timeout -k 10 280 rocprofv3 --pmc $K --kernel-trace -d $OUT/pmc/${C}_$K -o p --output-format csv -- python3 $R/bench.py --config $C --only --steps 2 --warmup 1 --full --no-cpu-baseline > $OUT/pmc/${C}_$K/run.log 2>&1
  done
  echo "$C done"
done
cd $R
python tools/trace_overlap.py $OUT/ks_C5 24 > $OUT/r03_C5_two_level_trace.txt
for C in C4 C5; do python bench.py --config $C --only --steps 10 --warmup 2 --full > $OUT/r03_bench_$C.json 2> $OUT/r03_bench_$C.err; done
python bench.py --full > $OUT/r03_bench_default.json 2> $OUT/r03_bench_default.err
