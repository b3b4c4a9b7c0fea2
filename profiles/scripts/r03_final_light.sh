#!/bin/bash
# round 3 evidence at HEAD: whole GPU suite, default bench line, profile recipe (kernel trace + PMC passes +
# traffic.json), phase stamps, the other workloads of the measured table
O=gpurun_out/$1; mkdir -p $O
export TMPDIR=/tmp
python py-swirld_amd/build.py --force > $O/build.log 2>&1 || { echo BUILD FAILED; tail -5 $O/build.log; exit 1; }
(timeout 1200 python -m pytest tests -m gpu -q > $O/pytest_gpu.log 2>&1; echo "pytest rc=$?" >> $O/pytest_gpu.log)
grep -E "^(FAILED|ERROR|[0-9]+ (passed|failed))|pytest rc" $O/pytest_gpu.log | cut -c1-300 | tail -12
timeout 300 python bench.py --full --steps 20 --warmup 5 > $O/bench_default.json 2> $O/bench_default.err
python -c "
import json; d=json.load(open('$O/bench_default.json')); print(d['value'], d['ms_per_step'], d['value_end_to_end'], d['roofline']['kernel'], d['roofline']['frac'], d['roofline']['path_frac'])
for k in d['roofline']['kernels']: print(k['kernel'], k['launches'], k['avg_launch_us'], k['total_ms'], k['frac'], k['hbm_bytes_per_launch_pmc'])"
SW_COMMIT=$(cat .commit_id 2>/dev/null || echo unknown) timeout 600 bash profiles/run_profiles.sh $1 > $O/prof.log 2>&1
head -12 gpurun_out/prof_$1/kernel_stats.txt; cat gpurun_out/prof_$1/loop_timeline.txt | head -6
SW_DEBUG_CLOCKS=1 SW_PIPE=1 timeout 120 python profiles/loop_phases.py 256 1000000 > $O/loop_phases_256x1M.txt 2>&1
B="--cpu-sample 0 --e2e-steps 0 --contexts 1"
timeout 200 python bench.py --full $B --steps 5 --warmup 2 --members 1024 --events 2000000 > $O/bench_1024x2M.json 2>> $O/err.log
timeout 200 python bench.py --full $B --steps 10 --warmup 2 --members 64 --events 100000 > $O/bench_64x100k.json 2>> $O/err.log
timeout 300 python bench.py --full $B --steps 3 --warmup 1 --mode 2 --p0 0.95 --p1 0.002 > $O/bench_hot_members_256x1M.json 2>> $O/err.log
timeout 300 python bench.py --full $B --steps 3 --warmup 1 --mode 2 --p0 0.35 --p1 0.02 > $O/bench_coin_stress_256x1M.json 2>> $O/err.log


python - $O <<'PY'
import json,glob,sys
for f in sorted(glob.glob(sys.argv[1]+"/bench_*.json")):
    try:
        d=json.load(open(f)); c=d["config"]
        print(f.split("/")[-1], "%.1f M ev/s  %.3f ms | rounds %d coin votes %d" % (d["value"]/1e6, d["ms_per_step"], c["rounds"], c["coin_round_votes"]))
    except Exception as e: print(f, "ERR", e)
PY
timeout 300 python profiles/incremental_bench.py > $O/incremental_small_batches.log 2>&1; head -2 $O/incremental_small_batches.log | cut -c1-300
