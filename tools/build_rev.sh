#!/bin/bash
# Build libtdec.so from the sources of a git revision (for in-process A/B with tools/ab.py):
#   tools/build_rev.sh <rev> <name> [-DDEFINE ...]  ->  modulations_amd/lib/libtdec_<name>.so
# The file list is the revision's own csrc listing, so older and newer layouts both build.
set -euo pipefail
rev=$1; name=$2; shift 2
d=$(mktemp -d)
mkdir -p $d/csrc $d/include modulations_amd/lib
for f in $(git ls-tree --name-only $rev modulations_amd/csrc/ | grep -E '/(tdec_[^/]*|npmath)\.hip$'); do
  git show $rev:$f > $d/csrc/$(basename $f)
done
for f in $(git ls-tree --name-only $rev include/ | grep -E '\.h$'); do   # tdec.h, and harq.h where the revision has it
  git show $rev:$f > $d/include/$(basename $f)
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -ffp-contract=off \
  -fno-gpu-flush-denormals-to-zero -w "$@" -I $d/include -o modulations_amd/lib/libtdec_$name.so $d/csrc/tdec_api.hip
rm -rf $d
echo modulations_amd/lib/libtdec_$name.so
