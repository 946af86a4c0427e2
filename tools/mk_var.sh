#!/bin/bash
# Build linkerd_amd/lib_ab/lib<name>.so from the working tree with extra compile
# flags (e.g. -DL5DH_PHASES for per-workgroup phase stamps).  Development tool.
#   tools/mk_var.sh <name> [hipcc flags...]
set -e
cd "$(dirname "$0")/../linkerd_amd/csrc"
N=$1; shift
F="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -ffp-contract=off -fno-fast-math -w -DL5DH_DEV $*"
T=$(mktemp -d)
mkdir -p ../lib_ab
for f in l5dh_ingest.hip l5dh_snapshot.hip l5dh_merge.hip l5dh_rollup.hip l5dh_le.hip l5dh_engine.cpp l5dh_fleet.cpp l5dh_tables.cpp; do
  /opt/rocm/bin/hipcc $F -x hip -c $f -o $T/${f%.*}.o &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../lib_ab/lib$N.so $T/*.o -L/opt/rocm/lib -lrccl
rm -rf $T
