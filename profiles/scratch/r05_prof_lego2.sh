#!/bin/bash
R=$PWD; export TMPDIR=/tmp; O=$(realpath -m "${1:?usage: profiles/scratch/r05_prof_lego2.sh <output dir>}"); mkdir -p $O
cd /tmp; rm -rf /tmp/prof_x
timeout 900 rocprofv3 --kernel-trace -d /tmp/prof_x -o p -- python3 $R/bench.py --full --workload lego --no-cpu-baseline --no-extras --no-traffic > $O/x.log 2>&1
db=$(find /tmp/prof_x -name '*.db' | head -1)
python3 $R/profiles/frame_launch_avgs.py $db > $O/frame_launch_avgs.txt
grep -o '"avg_launch_ms": [0-9.]*' $O/x.log | head -1 >> $O/frame_launch_avgs.txt
