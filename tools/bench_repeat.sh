# Fresh-process repeatability of the headline bench (placement probe verbose).
#   tools/bench_repeat.sh <tag> <runs> [extra bench args...]        (output under ${PROF_OUT:-prof_out}/<tag>)
set -euo pipefail
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
TAG=$1; RUNS=$2; shift 2
O=${PROF_OUT:-prof_out}/$TAG
mkdir -p $O
for i in $(seq 1 $RUNS); do
  TDEC_PROBE_VERBOSE=1 timeout -k 10 120 python -u bench.py --steps 3 --warmup 1 --full --no-cpu "$@" \
    > $O/run$i.json 2> $O/run$i.err
  grep -h "decode kernel" $O/run$i.err
done
