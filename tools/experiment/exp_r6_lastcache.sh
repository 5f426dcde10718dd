#!/bin/bash
# Round 6: the heap's last entry kept in the lane while it is known (MADSIM_HEAP_LAST_CACHE: after every push; the pop that follows loads nothing for it)
# against loading it at every pop (libmadsim_hip_nolast.so).  Narrow-heap builds: topology, election loop.
cd "$GRAFT_REPO_ROOT" || exit 1
O=gpurun_out/$1; mkdir -p "$O"
line() { python - "$1" "$2" <<'PY'
import json, sys
try:
    d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); e = d["extra"]
    print(sys.argv[2], "ms/step", round(d["ms_per_step"], 4), round(e["executor_steps_per_sec"] / 1e9, 3), "Gsteps/s kernel_ms", round(e["kernel_ms_per_step"], 3),
          "verified", d["verified_seeds"], "failed", e["failed_seeds"])
except Exception as ex:
    print(sys.argv[2], "NO LINE:", ex, open(sys.argv[1].replace(".json", ".err")).read()[-400:])
PY
}
run() { label=$1; wl=$2; steps=$3; shift 3
  env "$@" timeout 400 python bench.py --full --workload "$wl" --steps "$steps" --warmup 4 --no-cpu-baseline --no-measure-traffic --no-first-fail --no-extras \
    > "$O/x.json" 2> "$O/x.err"; line "$O/x.json" "$label"; }
NL=MADSIM_HIP_LIB=$PWD/madsim_amd/libmadsim_hip_nolast.so
timeout 1200 python -m pytest tests -m gpu -x -q > "$O/pytest.txt" 2>&1; tail -2 "$O/pytest.txt"
for round in 1 2 3 4; do
  run "topo last entry cached r$round" topo 16 X=1
  run "topo loaded at the pop r$round" topo 16 $NL
  run "raft last entry cached r$round" raft 20 X=1
  run "raft loaded at the pop r$round" raft 20 $NL
done | tee "$O/ab.txt"
