#!/bin/bash
# Round-end evidence on one MI355X: the full GPU parity suite, the headline
# bench (--full: with cpu_baseline) and every per-mode bench line, then
# rocprofv3 stats of the headline and of each mode.  Each step under its own
# limit.  Logs go to $OUT (default bench_out/).
set -u
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
export JY_PROGRESS=$PWD/$OUT/progress_${TAG:-r04}.log
TAG=${TAG:-r03}
if [ -z "${SKIP_TESTS:-}" ]; then
  timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 240 --timeout-method thread \
    > $OUT/pytest_gpu_$TAG.log 2>&1 || { tail -30 $OUT/pytest_gpu_$TAG.log; exit 1; }
  tail -1 $OUT/pytest_gpu_$TAG.log
fi
if [ -z "${SKIP_HEAD:-}" ]; then
  timeout -k 10 600 python bench.py --full > $OUT/bench_$TAG.log 2>&1 || { tail -20 $OUT/bench_$TAG.log; exit 1; }
  grep -h '^{' $OUT/bench_$TAG.log | cut -c1-400
fi
# UJSON warms up past its first pool compaction (sized from the state the
# setup converge built; later ones are ~50 converges apart)
wu() { [ "$1" = ujson ] && echo 6 || echo 2; }
for m in ${MODES-gcount treg tlog ujson e2e read}; do
  timeout -k 10 400 python bench.py --type $m --steps 8 --warmup $(wu $m) --full > $OUT/bench_${m}_$TAG.log 2>&1 || { tail -20 $OUT/bench_${m}_$TAG.log; exit 1; }
  grep -h '^{' $OUT/bench_${m}_$TAG.log | cut -c1-300
done
if [ -z "${SKIP_ROUTE:-}" ]; then
  timeout -k 10 400 python bench.py --type treg --route --steps 10 --warmup 3 > $OUT/bench_treg_route_$TAG.log 2>&1 || exit 1
  grep -h '^{' $OUT/bench_treg_route_$TAG.log | cut -c1-300
fi
if [ -n "${PROF:-}" ]; then
  [ -n "${SKIP_HEAD:-}" ] || timeout -k 10 500 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- python3 bench.py --steps 3 --warmup 1 --batches 2 > $OUT/prof_head_$TAG.log 2>&1 || exit 1
  for m in ${PMODES-gcount treg tlog ujson e2e read}; do
    timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_${m}_$TAG -o run --output-format csv -- python3 bench.py --type $m --steps 8 --warmup $(wu $m) > $OUT/prof_${m}_$TAG.log 2>&1 || exit 1
  done
fi
echo "round evidence done"
