#!/bin/bash
# Development aid: libegogen_hip.so with extra -D flags on ONE csrc file (default lbs_fused3.hip, the split-blend fused kernels) ->
# ab_libs/lib_<name>.so (the other objects as built)
#   bash scripts/build_variant.sh <name> "-DEGX_LBS_NOFIX ..." [report] [file.hip]
set -eu
R=$(cd "$(dirname "$0")/.." && pwd)
N=$1; FL=${2:-}; REP=${3:-}; F=${4:-lbs_fused3.hip}
B=${F%.hip}
mkdir -p $R/ab_libs $R/build
make -s -C $R/egogen_amd/csrc > /dev/null
EXTRA=""
[ -n "$REP" ] && EXTRA="-Rpass-analysis=kernel-resource-usage"
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function $FL $EXTRA -c $R/egogen_amd/csrc/$F -o $R/build/${B}_$N.o 2> $R/build/${B}_$N.log || { tail -20 $R/build/${B}_$N.log; exit 1; }
OBJS=$(ls $R/egogen_amd/csrc/*.o | grep -v "/$B.o")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $OBJS $R/build/${B}_$N.o -o $R/ab_libs/lib_$N.so
ls -la $R/ab_libs/lib_$N.so
