#!/bin/bash
R=$PWD; export TMPDIR=/tmp; O=$(realpath -m "${1:?usage: profiles/scratch/r05_prof_lego.sh <output dir>}"); mkdir -p $O
cd /tmp
name=bench_lego
rm -rf /tmp/prof_$name
timeout 900 rocprofv3 --kernel-trace --stats -d /tmp/prof_$name -o p -- python3 $R/bench.py --full --workload lego --no-cpu-baseline --no-extras --no-traffic > $O/$name.log 2>&1
db=$(find /tmp/prof_$name -name '*.db' | head -1)
{ echo "# rocprofv3 --kernel-trace --stats -- python3 bench.py --full --workload lego --no-cpu-baseline --no-extras --no-traffic   (round 5; bench.py's default steps / warmup)"; python3 $R/profiles/summarize.py $db;
  grep -o '"avg_launch_ms": [0-9.]*' $O/$name.log | head -1 | sed 's/^/# the same run, bench.py line (HIP events carried by the working lookup launches of the first timed step): /';
  grep -o '"frac": [0-9.]*' $O/$name.log | head -1 | sed 's/^/# the same run, bench.py line roofline /';
  python3 $R/profiles/frame_launch_avgs.py $db 5 20 | grep "^#"; } > $O/$name.txt
for wl in lego_palette garden; do
  name=bench_$wl; rm -rf /tmp/prof_$name
  timeout 900 rocprofv3 --kernel-trace --stats -d /tmp/prof_$name -o p -- python3 $R/bench.py --full --workload $wl --steps 10 --warmup 3 --no-cpu-baseline --no-extras --no-traffic > $O/$name.log 2>&1
  db=$(find /tmp/prof_$name -name '*.db' | head -1)
  { echo "# rocprofv3 --kernel-trace --stats -- python3 bench.py --full --workload $wl --steps 10 --warmup 3 --no-cpu-baseline --no-extras --no-traffic   (round 5)"; python3 $R/profiles/summarize.py $db; } > $O/$name.txt
done
