#!/bin/bash
# usage: tools/profile_round.sh <tag> <mesh>: rocprofv3 kernel stats + three PMC passes of bench.py (run on the GPU box)
# output: $CFX_PROFILE_OUT (default prof_out/ in the repository), read by tools/collect_profiles.sh
set -eu
TAG=$1; N=$2
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
OUT=${CFX_PROFILE_OUT:-$R/prof_out}
mkdir -p $OUT
cd /tmp
export CFX_BENCH_DETAIL=prof_${TAG}_bench_detail.json CFX_BENCH_PRINT_DETAIL=1
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG} -- python3 $R/bench.py --full --mesh $N --steps 10 --warmup 2 --no-cpu --no-secondary > $OUT/prof_${TAG}_bench.json 2> $OUT/prof_${TAG}.err
sed -n 's/^# bench_detail: //p' $OUT/prof_${TAG}.err > $OUT/prof_${TAG}_bench_detail.json
export CFX_BENCH_PRINT_DETAIL=0
echo stats done
rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAIT_ANY SQ_WAIT_INST_ANY --output-format csv -d $OUT/pmc_${TAG}_sq -- python3 $R/bench.py --full --mesh $N --steps 2 --warmup 1 --no-cpu --no-secondary > /dev/null 2> $OUT/pmc_${TAG}_sq.err
echo sq done
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_${TAG}_fetch -- python3 $R/bench.py --full --mesh $N --steps 2 --warmup 1 --no-cpu --no-secondary > /dev/null 2> $OUT/pmc_${TAG}_fetch.err
echo fetch done
rocprofv3 --kernel-trace --pmc WRITE_SIZE TCC_HIT_sum TCC_MISS_sum --output-format csv -d $OUT/pmc_${TAG}_write -- python3 $R/bench.py --full --mesh $N --steps 2 --warmup 1 --no-cpu --no-secondary > /dev/null 2> $OUT/pmc_${TAG}_write.err
echo write done
python3 $R/tools/pmc_report.py $OUT/pmc_${TAG}_sq $OUT/pmc_${TAG}_fetch $OUT/pmc_${TAG}_write > $OUT/pmc_${TAG}_summary.txt
