#!/bin/bash
# Round evidence on the GPU box (repo root): GPU tests, rocprofv3 kernel trace + PMC passes of
# the bench workload, their summary into profiles/ (PMC traffic per wf_trace launch), then the
# driver's bench command with --full (which reads that summary).  Everything lands in
# $RT_OUT_DIR (default out/), the new profiles/ files in $RT_OUT_DIR/profiles.
set -o pipefail
export TMPDIR=/tmp
TAG=${TAG:-r05_C3}
O=${RT_OUT_DIR:-out}
mkdir -p $O/profiles
timeout -k 10 600 python3 -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $O/pytest_gpu.log 2>&1 || { echo "gpu tests failed"; tail -30 $O/pytest_gpu.log; exit 1; }
tail -2 $O/pytest_gpu.log
bash tools/profile_gpu.sh $O/prof || { echo "profile failed"; exit 1; }
python3 tools/summarize_profile.py $O/prof $TAG \
  '{"config": "C3", "width": 1920, "height": 1080, "frames_per_step": 1024, "path_slots_per_rank": 2139095040, "probe_trace_launches": 9, "command": "bash tools/profile_gpu.sh (bench.py --full --steps 3 --warmup 1 --cpu-seconds 0 --single-frames 0)"}' > $O/summary.log || exit 1
timeout -k 10 600 python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $O/bench.json 2> $O/bench.err || { echo "bench failed"; tail -20 $O/bench.err; exit 1; }
cat $O/bench.json
cp $O/bench.json $O/profiles/${TAG%_C3}_bench_C3.json
cp profiles/${TAG}_* profiles/pmc_C3.json $O/profiles/
[ -n "$SKIP_INTERACTIVE" ] && exit 0
timeout -k 10 300 python3 tools/interactive_demo.py --config C3 --frames 60 --out $O/interactive > $O/interactive.log 2>&1 || { echo "interactive failed"; tail -5 $O/interactive.log; exit 1; }
cp $O/interactive/C3_interactive.json $O/profiles/${TAG}_interactive.json
tail -7 $O/interactive.log
timeout -k 10 300 python3 tools/interactive_demo.py --config C3 --frames 60 --in-flight 2 --out $O/interactive2 > $O/interactive2.log 2>&1 || { echo "interactive (2 in flight) failed"; tail -5 $O/interactive2.log; exit 1; }
cp $O/interactive2/C3_interactive.json $O/profiles/${TAG}_interactive_in_flight2.json
tail -7 $O/interactive2.log
