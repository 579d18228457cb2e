#!/bin/bash
# Round-3 profile of one bench configuration: bench line + kernel trace + PMC passes
#   tools/prof_config.sh <tag> <bench args...>        (output under ${PROF_OUT:-prof_out}/<tag>)
set -o pipefail
cd /tmp && export TMPDIR=/tmp && cd - > /dev/null
TAG=$1
shift
O=${PROF_OUT:-prof_out}/$TAG
mkdir -p $O
timeout -k 10 400 python -u bench.py --full --no-cpu "$@" > $O/bench.json 2> $O/bench.err || exit $?
tools/profile.sh $TAG python bench.py --steps 1 --warmup 1 "$@"
