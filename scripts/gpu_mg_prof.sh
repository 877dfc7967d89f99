#!/bin/bash
# rocprofv3 kernel stats + trace of the MG-PCG solve workload (512^3)
set -u
R=$GRAFT_REPO_ROOT
O=${PB_OUT_DIR:-$R/out}  # where the job writes
mkdir -p $O/mgprof
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/mgprof -o mg --output-format csv -- python3 $R/bench.py --full --workload star7-mg --steps 2 --warmup 1 --cpu-baseline none > $O/mgprof/bench.json 2> $O/mgprof/bench.err
echo "rc=$?"
