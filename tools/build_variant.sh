#!/bin/bash
# Diagnostic build of libpqgpu.so with extra defines (A/B experiments; loaded through PQGPU_LIB):
#   bash tools/build_variant.sh abx/libnoval.so -DPQG_XT_NOVALUE
set -euo pipefail
OUT=$(realpath -m "$1"); shift
cd "$(dirname "$0")/.."  # the repository root: the paths below and __graft_entry__ are relative to it
C=parquet-mr_amd/csrc
# the source list of build() (__graft_entry__.SOURCES), so there is no second one to keep
SRC=$(python3 -c 'import __graft_entry__ as g; print(" ".join("'$C'/" + f for f in g.SOURCES))')
mkdir -p "$(dirname "$OUT")"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wall -shared "$@" -o "$OUT" $SRC -Wl,--no-undefined
