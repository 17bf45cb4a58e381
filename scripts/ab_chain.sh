#!/bin/bash
# A/B of the swap chain's depth on the headline (T-Rex 1024^2), in the environment as it is found —
# GPU_MAX_HW_QUEUES is NOT set here except for the ceiling runs.  Alternates, REPS times (default 5), at the
# bench defaults (K = 200, W = 20) and at the driver's K = 20, W = 5:
#   parent    `python bench.py` of another built tree (PARENT=<its root>; skipped when unset)
#   shared    `python bench.py`                       the filler's own choice: depth 4, slot 3 on the caller's stream
#   depth3    `python bench.py --pipeline-depth 3`    same tree, three frames in flight (the control)
#   ceiling   `GPU_MAX_HW_QUEUES=8 python bench.py`   depth 4 on four streams of the chain's own, a queue each
# then cube256 and bunny4096 once each.  One line per run; a summary (median, min - max) at the end.
# Every run has a time limit of its own, and the first one that fails ends the script.
set -o pipefail
cd "$(dirname "$0")/.."
HERE=$(pwd)
REPS=${REPS:-5}
line() { python -c "
import json,sys
tag=sys.argv[1]
ok=False
for l in sys.stdin:
    if l.startswith('{'):
        d=json.loads(l); ok=True
        print('%-8s %-10s K=%-4d fps=%10.1f ms=%7.4f | %s' % (tag, d['config']['workload'], d['steps'], d['value'], d['ms_per_step'], str(d['config']['pipelined'])[:44]))
sys.exit(0 if ok else 1)" "$1"; }
run() {  # tag, directory, extra environment (or ""), bench arguments
  local tag=$1 dir=$2 env=$3; shift 3
  ( cd "$dir" && env $env timeout -k 10 180 python bench.py "$@" 2>/dev/null ) | line "$tag" | tee -a "$OUT"
}
OUT=$(mktemp)
for kw in "--steps 200 --warmup 20" "--steps 20 --warmup 5"; do
  for rep in $(seq "$REPS"); do
    if [ -n "${PARENT:-}" ]; then run parent "$PARENT" "" $kw || exit 1; fi
    run shared "$HERE" "" $kw || exit 1
    run depth3 "$HERE" "" $kw --pipeline-depth 3 || exit 1
    run ceiling "$HERE" "GPU_MAX_HW_QUEUES=8" $kw || exit 1
  done
done
for wl in cube256 bunny4096; do
  if [ -n "${PARENT:-}" ]; then run parent "$PARENT" "" --workload $wl || exit 1; fi
  run shared "$HERE" "" --workload $wl || exit 1
done
python - "$OUT" <<'EOF'
import re, statistics, sys
runs = {}
for l in open(sys.argv[1]):
    m = re.match(r"(\w+)\s+(\w+)\s+K=(\d+)\s+fps=\s*([\d.]+)", l)
    if m:
        runs.setdefault((m.group(2), int(m.group(3)), m.group(1)), []).append(float(m.group(4)))
print("summary: frames/s, median (min - max) of n runs")
med = {}
for (wl, K, tag), v in sorted(runs.items()):
    med[(wl, K, tag)] = statistics.median(v)
    print(f"  {wl:<10} K={K:<4} {tag:<8} {statistics.median(v):10.1f} ({min(v):10.1f} - {max(v):10.1f}) n={len(v)}")
for (wl, K, tag), m in sorted(med.items()):
    if tag == "shared":
        for other in ("parent", "depth3", "ceiling"):
            if (wl, K, other) in med:
                print(f"  {wl:<10} K={K:<4} shared / {other:<8} = {m / med[(wl, K, other)]:.3f}")
EOF
rm -f "$OUT"
