#!/bin/bash
# End-of-round measurement on the GPU box: full GPU suite, the default bench line, and the rocprofv3 kernel stats of (a) the default bench
# command and (b) the one-in-flight configuration the roofline is quoted on.  Results under $OUT/<tag>_*; copy into profiles/.
set -o pipefail
R=${GRAFT_REPO_ROOT:-/root/repo}; T=${1:-final}
OUT=${OUT:-$R/out}; mkdir -p "$OUT"          # where the logs, JSON lines and profiles go
cd $R
python -m pytest tests -m gpu -x -q > $OUT/${T}_tests.log 2>&1 || { tail -n 30 $OUT/${T}_tests.log; exit 1; }
tail -n 2 $OUT/${T}_tests.log
python bench.py --full > $OUT/${T}_bench_default.json 2> $OUT/${T}_bench_default.err || exit 2
cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${T}_prof_default -o runc -- python3 $R/bench.py --full --no-cpu-baseline --no-config5 > $OUT/${T}_bench_profiled.json 2> $OUT/${T}_bench_profiled.err || exit 3
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${T}_prof_nopipe -o runc -- python3 $R/bench.py --full --no-pipeline --no-extras --no-prove --no-cpu-baseline > $OUT/${T}_bench_nopipe.json 2> $OUT/${T}_bench_nopipe.err || exit 4
cd $R
python tools/show_bench.py $OUT/${T}_bench_default.json $OUT/${T}_bench_profiled.json $OUT/${T}_bench_nopipe.json
