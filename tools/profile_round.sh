#!/bin/bash
# One profiling pass of the default bench on an MI355X:
#   bash tools/profile_round.sh r01e [all|bench|pmc] [OUT]
# writes OUT/<tag>_bench.json (bench.py --full), OUT/prof_<tag>/ (kernel-trace stats) and OUT/pmc_<tag>_{fetch,write}/
# (HBM counters, one rocprofv3 pass each, never combined with a trace domain); OUT defaults to profile_out/ in the repository.
# tools/pmc_traffic.py turns the counter CSVs into profiles/<tag>_pmc_traffic.json
# (python tools/pmc_traffic.py OUT/pmc_<tag>_fetch OUT/pmc_<tag>_write 4096 f16x3).
set -e
TAG=${1:-round}
WHAT=${2:-all}   # all | bench (bench + kernel stats) | pmc (the two counter passes)
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "${3:-$R/profile_out}"
OUT=$(cd "${3:-$R/profile_out}" && pwd)
cd $R
if [ $WHAT != pmc ]; then
timeout -k 10 600 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
echo BENCH_DONE
cd /tmp && export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG} -o ${TAG} -- python $R/bench.py --steps 3 --warmup 1 --no-prof > $OUT/${TAG}_prof_bench.json 2> $OUT/${TAG}_prof.err
echo STATS_DONE
fi
if [ $WHAT = bench ]; then exit 0; fi
cd /tmp && export TMPDIR=/tmp
timeout -k 10 900 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_${TAG}_fetch -o ${TAG} -- python $R/bench.py --steps 1 --warmup 1 --no-prof > /dev/null 2> $OUT/${TAG}_pmc_fetch.err
echo FETCH_DONE
timeout -k 10 900 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_${TAG}_write -o ${TAG} -- python $R/bench.py --steps 1 --warmup 1 --no-prof > /dev/null 2> $OUT/${TAG}_pmc_write.err
echo WRITE_DONE
rm -f $OUT/prof_${TAG}/*kernel_trace.csv   # (large; the stats CSV is what is kept)
ls $OUT/pmc_${TAG}_fetch $OUT/pmc_${TAG}_write
