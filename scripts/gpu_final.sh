#!/bin/bash
# End-of-round check: every GPU test, smoke(), the whole bench record (--full),
# and the headline's rocprofv3 profile (trace + FETCH/WRITE/L2 passes).
# Logs go to OUT_DIR (default bench_out).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
O=${OUT_DIR:-bench_out}
mkdir -p "$O"
T=${TAG:-final}
timeout -k 10 900 python -u -m pytest -v --timeout 400 --timeout-method thread -m gpu tests > "$O/${T}_tests.log" 2>&1
rc=$?; echo "[tests] exit $rc" | tee -a "$O/${T}_status.log"; [ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > "$O/${T}_smoke.log" 2>&1
rc=$?; echo "[smoke] exit $rc" | tee -a "$O/${T}_status.log"; [ $rc -ne 0 ] && exit $rc
timeout -k 10 400 python -u bench.py --full > "$O/${T}_bench.log" 2>&1
rc=$?; echo "[bench] exit $rc" | tee -a "$O/${T}_status.log"; [ $rc -ne 0 ] && exit $rc
[ -n "${NO_PROF:-}" ] && exit 0
PROF_TAG=${T}_prof bash scripts/profile.sh
