#!/bin/bash
# Build a variant of the library with extra -D flags into gpurun_out/ and run a pytest selection against it.
# usage: tools/test_variant.sh "<-D flags>" <pytest -k expression>
ROOT=$(cd $(dirname $0)/.. && pwd)
FLAGS=$1; shift
LIB=$ROOT/gpurun_out/lib_variant.so
mkdir -p $ROOT/gpurun_out
(cd $ROOT && python -m waveglow_amd.build -o $LIB $FLAGS) || exit 1
WAVEGLOW_AMD_LIB=$LIB timeout -k 10 300 python -m pytest $ROOT/tests -m gpu -x -q -k "$*" 2>&1 | tail -4
