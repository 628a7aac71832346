#!/bin/bash
# A/B kernel variants on one box: alternates bench.py runs over the given
# library builds (GS_LIB_PATH) and prints per-stage times.
# usage: tools/ab.sh <rounds> <lib.so> [<lib.so> ...]   (run from the repo root)
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
rounds=$1; shift
mkdir -p "$R/gpurun_out/ab"
for ((i = 0; i < rounds; i++)); do
  for lib in "$@"; do
    n=$(basename "$lib" .so)
    GS_LIB_PATH=$R/$lib timeout -k 10 200 python "$R/bench.py" --full --steps 10 --warmup 2 --no-cpu-baseline \
      > "$R/gpurun_out/ab/${n}_$i.log" 2>&1 || { echo "bench failed: $lib"; exit 1; }
    python3 - "$R/gpurun_out/ab/${n}_$i.log" "$n" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
s = d["stages_ms"]
print(f"{sys.argv[2]:24s} ms/step {d['ms_per_step']:.4f} " + " ".join(f"{k}={v:.4f}" for k, v in s.items()), flush=True)
PY
  done
done
