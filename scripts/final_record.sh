# GPU box: the closing record of a round after the last source change -- full GPU test suite, the default bench line, the PMC
# traffic files keyed on this build (profiles/r04_pmc_*.json) and the two-rank gloo rehearsal of the streamed scatter leg.
# The two bench lines (bench.py --full) go to $RECORD_DIR (default records/); the test log and the PMC passes go where
# scripts/pmc_run.sh writes its own outputs.
set -euo pipefail
cd $GRAFT_REPO_ROOT
OUT=${RECORD_DIR:-records}
mkdir -p "$OUT"
python -m pytest tests -m gpu -x -q > gpurun_out/t_full_final.log 2>&1
tail -2 gpurun_out/t_full_final.log
timeout -k 10 600 python bench.py --full > "$OUT/c_bench_slab_stage1.log" 2>&1
tail -1 "$OUT/c_bench_slab_stage1.log" | cut -c1-160
bash scripts/pmc_run.sh > gpurun_out/pmc_run.log 2>&1
tail -5 gpurun_out/pmc_run.log
rm -rf gpurun_out/pmc_fetch gpurun_out/pmc_write
timeout -k 10 500 python bench.py --gpus 2 --backend gloo --share-gpu --bl 8 --steps 2 --warmup 1 --full --no-other-params --no-other-workloads --no-cpu-baseline > "$OUT/c_gloo2.log" 2>&1
tail -1 "$OUT/c_gloo2.log" | cut -c1-200
