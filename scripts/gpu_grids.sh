#!/bin/bash
# per-GPU slab shapes of the weak-scaling runs (N = 1, 4, 8), interleaved, one process each
set -u
O=${PB_OUT_DIR:-out}  # where the job writes
mkdir -p $O
for g in 512,512,512 1024,1024,128 512,1024,256 1024,1024,128 512,512,512 1024,1024,128; do
  timeout -k 10 200 python bench.py --full --grid $g --steps 40 --warmup 5 --secondary 0 --cpu-baseline none > $O/grid.json 2> $O/grid.err || exit 1
  python scripts/show_grid.py $g $O/grid.json >> $O/grids.txt
done
cat $O/grids.txt
