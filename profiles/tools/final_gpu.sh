# Round-end check on the GPU box: full GPU suite, the bench line, and the rocprofv3 kernel stats of the headline
# command (no secondary workloads, so the dominant kernel's average is the one bench.py reports).
#   bash profiles/tools/final_gpu.sh OUTDIR     (logs and the bench line go to OUTDIR)
set -e
cd $GRAFT_REPO_ROOT
OUT=${1:?usage: final_gpu.sh OUTDIR}; mkdir -p "$OUT"
timeout -k 10 900 python -m pytest tests -x -q -m gpu > "$OUT/gpu_tests.log" 2>&1; tail -2 "$OUT/gpu_tests.log"
timeout -k 10 600 python bench.py --full > "$OUT/bench_final.json" 2> "$OUT/bench_final.err"
python profiles/benchline.py "$OUT/bench_final.json"
bash profiles/tools/profile_headline.sh
