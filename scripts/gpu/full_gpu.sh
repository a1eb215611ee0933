# whole GPU test suite + smoke + 1-GPU bench with its extras; logs go to $LOGS
set -o pipefail
LOGS=${LOGS:-logs}
mkdir -p "$LOGS"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > "$LOGS/full_gpu.log" 2>&1 &&
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke(); print('SMOKE OK')" > "$LOGS/full_smoke.log" 2>&1 &&
timeout -k 10 600 python -u bench.py --full > "$LOGS/full_bench.log" 2>&1
