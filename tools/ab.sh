#!/bin/bash
# Same-box A/B of the step time: HEAD (exported into _ab/, built there) against the working tree.  Boxes differ by ~2 %
# (clocks, DVFS), so a change below that only shows in a same-box comparison.
#   here:        bash tools/ab.sh prepare          (git archive HEAD -> _ab/, build)
#   on the box:  bash tools/ab.sh run     (ROUNDS alternating rounds, default 3, of bench.py --steps 20)
#                bash tools/ab.sh scene   (the same for tools/bench_scene.py, the config-5 step)
set -e -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
cd "$R"
if [ "$1" = "prepare" ]; then
  rm -rf _ab && mkdir -p _ab && git archive HEAD | tar -x -C _ab
  (cd _ab && python3 -c "
import importlib,sys
sys.path.insert(0,'.')
print(importlib.import_module('single-view-3d-reconstruction_amd.build').build())")
  exit 0
fi
one() { timeout -k 10 300 python3 bench.py --steps 20 --warmup 5 --no-cpu-baseline --no-query --no-diag --no-fwd-only 2>/dev/null | python3 -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$1', round(d['ms_per_step'],3), round(d['step_ms']['median'],3))"; }
scene() { timeout -k 10 300 python3 tools/bench_scene.py --steps 20 2>/dev/null | python3 -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$1', round(d['ms_per_step'],3), round(d['step_ms']['median'],3))"; }
for i in $(seq ${ROUNDS:-3}); do
  if [ "$1" = "scene" ]; then (cd _ab && scene "HEAD   "); scene "working"; else (cd _ab && one "HEAD   "); one "working"; fi
done
