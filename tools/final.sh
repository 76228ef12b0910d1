#!/bin/bash
# validation of a tree in two calls (each stays under 20 minutes):
#   tools/final.sh TAG tests  -> every -m gpu test + smoke
#   tools/final.sh TAG bench  -> default bench (--full), configs 2 / 3, file pipeline
# logs go to $OF_OUT (default out/)
set -u
TAG=${1:-final}
PART=${2:-tests}
export PYTHONDONTWRITEBYTECODE=1
O=${OF_OUT:-out}
mkdir -p $O
if [ "$PART" = tests ]; then
tools/gpu_step.sh 1000 $O/${TAG}_gpu.log python -u -m pytest -v -rA --timeout 300 --timeout-method thread tests -m gpu && \
tools/gpu_step.sh 150 $O/${TAG}_smoke.log python -u -c "import __graft_entry__ as g; g.smoke()"
else
tools/gpu_step.sh 400 $O/${TAG}_bench.log python -u bench.py --full && \
tools/gpu_step.sh 250 $O/${TAG}_bench_cfg2.log python -u bench.py --full --method hs --solver sor --height 480 --width 640 && \
tools/gpu_step.sh 250 $O/${TAG}_bench_cfg3.log python -u bench.py --full --method classic-c --solver pcg --height 720 --width 1280 && \
tools/gpu_step.sh 300 $O/${TAG}_pipeline.log python -u tools/pipeline_bench.py --pairs 48
fi
