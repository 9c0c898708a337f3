#!/bin/bash
# round 6: smoke + the bench run with --full (committed as profiles/round6_bench_default_run.json); the GPU suite ran in r6_tests_collect.sh
cd "$GRAFT_REPO_ROOT"; mkdir -p gpurun_out
OUT=$_                   # bash: the last argument of the command above, i.e. the folder it made
timeout 600 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | grep -v amdgpu | tail -2 > gpurun_out/r6_final_smoke.txt
timeout 1200 python bench.py --full > $OUT/r6_bench_default_run.json 2> $OUT/r6_bench_default_run.err
cat gpurun_out/r6_final_smoke.txt; cut -c1-900 gpurun_out/r6_bench_default_run.json
