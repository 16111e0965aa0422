#!/bin/bash
# A/B timing of library builds (LIBS: "cur" = the in-tree library, NAME =
# exp/libsyzsig_NAME.so), alternating, two runs each: ms/step, the scatter
# stage and the Minimize line (bench.py --full).  Logs go to OUT_DIR/minab
# (OUT_DIR defaults to bench_out).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
O=${OUT_DIR:-bench_out}/minab
mkdir -p "$O"
for i in 1 2; do for lib in ${LIBS:-base cur}; do
	if [ "$lib" = cur ]; then unset SYZSIG_LIB; else export SYZSIG_LIB=exp/libsyzsig_$lib.so; fi
	timeout -k 10 300 python3 bench.py --full --steps 10 --warmup 2 --no-cpu > "$O/$lib$i.log" 2>&1 || exit 1
	echo "$lib $i $(tail -1 "$O/$lib$i.log" | python3 -c 'import json,sys; d=json.loads(sys.stdin.read()); print("ms/step %.3f part %.3f agg %.3f min %.3f" % (d["ms_per_step"], d["stages"]["part_ms"], d["stages"]["agg_ms"], d["lines"]["minimize"]["ms"]))')" | tee -a "$O/summary.txt"
done; done
