#!/bin/bash
# Build a variant of the library with extra -D flags (cross-compiles without a GPU): tools/build_variant.sh <name> "<flags>"
# -> build_variants/lib_<name>.so (*.so is git-ignored).  Fails on VGPR spills / scratch, like the in-tree build.
ROOT=$(cd $(dirname $0)/.. && pwd)
mkdir -p $ROOT/build_variants
cd $ROOT && python -m waveglow_amd.build -o $ROOT/build_variants/lib_$1.so $2 || exit 1
