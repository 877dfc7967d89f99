#!/bin/bash
# A/B of library variants (variants/<name>.so, scripts/build_variant.sh) on the default bench line,
# interleaved: usage  V="base pa2 pa3" bash scripts/gpu_ab_lib.sh
set -u
O=${PB_OUT_DIR:-out}  # where the job writes
mkdir -p $O
: > $O/ab_lib.txt
for rep in 1 2; do
  for v in ${V:-base}; do
    if [ $v = base ]; then unset PB_LIB; else export PB_LIB=variants/$v.so; fi
    timeout -k 10 200 python bench.py --full --steps 40 --warmup 5 --secondary 0 --cpu-baseline none > $O/ab.json 2> $O/ab.err || exit 1
    python scripts/show_grid.py $v $O/ab.json >> $O/ab_lib.txt
  done
done
cat $O/ab_lib.txt
