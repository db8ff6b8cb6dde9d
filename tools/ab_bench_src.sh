#!/bin/bash
# A/B the in-tree library (A) against a build of another checkout of this repository (B) on ONE box, interleaved.
# usage: tools/ab_bench_src.sh <root of the checkout of variant B> [bench args]     (B is built by its own waveglow_amd.build,
# which has the command line from the commit that removed the ablation switches on; an older checkout builds nothing and is refused)
ROOT=$(cd $(dirname $0)/.. && pwd)
SRC=$1; shift
LIB=$ROOT/gpurun_out/lib_variantB.so
mkdir -p $ROOT/gpurun_out
rm -f $LIB
(cd $SRC && python -m waveglow_amd.build -o $LIB) || exit 1
[ -f $LIB ] || { echo "$SRC: python -m waveglow_amd.build built no library (a checkout without the build command line?)"; exit 1; }
for round in 1 2 3; do
  for v in A B; do
    if [ $v = A ]; then unset WAVEGLOW_AMD_LIB; else export WAVEGLOW_AMD_LIB=$LIB; fi
    timeout -k 10 300 python $ROOT/bench.py --full --no-cpu-baseline --no-secondary --steps 10 --warmup 3 "$@" 2>/dev/null | python -c "
import sys, json
for l in sys.stdin:
  if l.startswith('{'):
    d = json.loads(l); r = d['roofline']
    print('$v round $round: %.3f ms/step  wn_layer avg %.4f ms  frac %.4f' % (d['ms_per_step'], r['avg_launch_ms'], r['frac']))
"
  done
done
