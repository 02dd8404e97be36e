# PMC passes over the fused 2-hop count's P1 and P3 (not a test), each counter
# set in a run of its own, no tracing combined.  bench.py drives: the first
# query builds the in-side index, the others probe it.
#   tools/pmc_p3.sh [TAG]      output: $PMC_OUT[_TAG]/{fetch,write,tcc} (PMC_OUT: bench_out/pmc_p3 unless set)
# CAPF_LIB_AB in the environment selects the build (A/B of two libraries).
# tools/make_pmc_json.py $PMC_OUT[_TAG] 24 then assembles the bytes per query.
set -e
OUT=${PMC_OUT:-bench_out/pmc_p3}${1:+_$1}
mkdir -p $OUT
RX="c5_partition|c5_gather"
DRIVE="python3 bench.py --gpus 1 --steps 3 --warmup 1 --no-cpu"
timeout -k 10 120 rocprofv3 --kernel-include-regex "$RX" --pmc FETCH_SIZE -d $OUT/fetch -o f --output-format csv -- $DRIVE > $OUT/fetch.log 2>&1
timeout -k 10 120 rocprofv3 --kernel-include-regex "$RX" --pmc WRITE_SIZE -d $OUT/write -o w --output-format csv -- $DRIVE > $OUT/write.log 2>&1
timeout -k 10 120 rocprofv3 --kernel-include-regex "$RX" --pmc TCC_HIT_sum TCC_MISS_sum -d $OUT/tcc -o t --output-format csv -- $DRIVE > $OUT/tcc.log 2>&1
echo done $OUT
