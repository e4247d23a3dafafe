R=$PWD; export TMPDIR=/tmp
O=$(realpath -m "${1:?usage: profiles/scratch/prof_garden_only.sh <output dir>}"); mkdir -p $O
cd /tmp; rm -rf /tmp/prof_bench_garden
rocprofv3 --kernel-trace --stats -d /tmp/prof_bench_garden -o p -- python3 $R/bench.py --full --workload garden --steps 10 --warmup 3 --no-cpu-baseline --no-extras > /dev/null 2>&1
{ echo "# rocprofv3 --kernel-trace --stats -- python3 bench.py --full --workload garden --steps 10 --warmup 3 --no-cpu-baseline --no-extras   (round 3)"; python3 $R/profiles/summarize.py $(find /tmp/prof_bench_garden -name '*.db' | head -1); } > $O/bench_garden.txt
head -9 $O/bench_garden.txt | cut -c1-120
