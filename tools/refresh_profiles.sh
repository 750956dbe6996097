set -u
# usage: [ROUND=r2] [OUT=dir] tools/refresh_profiles.sh   (bench line, kernel stats under rocprofv3 for the SAME command, PMC passes -> $OUT/$ROUND)
R=$PWD
O=$R/${OUT:-out}/${ROUND:-r03}
mkdir -p $O
python bench.py --full > $O/bench_T1000.json 2> $O/bench_T1000.err
cat $O/bench_T1000.json
cd /tmp && export TMPDIR=/tmp
# the SAME timed region as the headline bench line (python bench.py: T=1000, 3 steps + 1 warm-up) under the kernel tracer; the
# secondary blocks of --full that run AFTER the timed region (parity / T=100 / cpu baseline / training line) are left out because they
# launch the same kernel name with other shapes and would pollute its average
rocprofv3 --kernel-trace --stats -d $O/kstats --output-format csv -- python $R/bench.py > $O/kstats.log 2>&1
cd $R
find $O/kstats -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $O/kernel_stats.csv
head -6 $O/kernel_stats.csv
grep "^{" $O/kstats.log | tail -1 | tee $O/bench_under_prof.json | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('bench line under rocprofv3: kernel_ms', d['roofline']['kernel_ms'], 'value', d['value'])"
tools/prof_pmc.sh $O/pmc --timesteps 20 --steps 1 --warmup 1
