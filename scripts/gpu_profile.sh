#!/bin/bash
# Profiling helper: the round's measured artefacts on the GPU.  usage: gpu_profile.sh <tag> [<output dir>, default profile_out]
#   1. bench.py --full (default config, with cpu_baseline)     -> <output dir>/bench_<tag>.json
#   2. rocprofv3 --kernel-trace --stats of the same command    -> <output dir>/prof_<tag>/
#   3. PMC passes (separate runs, counters only): HBM bytes, MFMA busy
# (the default bench.py --full run holds only full-matrix launches of every GEMM kernel, so per-kernel averages are per-launch figures;
#  2 and 3 keep --full for the other GEMM paths and residencies, whose kernels the PMC table and bench.py's pmc_traffic look up)
tag=$1
out=${2:-profile_out}
mkdir -p "$out"
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
timeout -k 10 500 python bench.py --full > "$out/bench_$tag.json" 2> "$out/bench_$tag.err" || tail -5 "$out/bench_$tag.err"
rocprofv3 --kernel-trace --stats --output-format csv -d "$out/prof_$tag" -- python bench.py --full --no-cpu-baseline --no-extras > "$out/prof_$tag.log" 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$out/pmc_fetch_$tag" -- python bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-extras > "$out/pmc_fetch_$tag.log" 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$out/pmc_write_$tag" -- python bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-extras > "$out/pmc_write_$tag.log" 2>&1
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY GRBM_GUI_ACTIVE --output-format csv -d "$out/pmc_sq_$tag" -- python bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-extras > "$out/pmc_sq_$tag.log" 2>&1
python scripts/summarize_profile.py $tag "$out"
