#!/bin/bash
# Build linkerd_amd/lib_ab/lib<name>.so from the working tree with extra compile
# flags (e.g. -DL5DH_PHASES for per-workgroup phase stamps).  Development tool.
# The sources and the base flags are the Makefile's.
#   tools/mk_var.sh <name> [hipcc flags...]
set -e
cd "$(dirname "$0")/../linkerd_amd/csrc"
N=$1; shift
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
make -s -j16 OUT="$T" EXTRA="-w $*" "$T/libl5dhist.so"
mkdir -p ../lib_ab
cp "$T/libl5dhist.so" ../lib_ab/lib$N.so
