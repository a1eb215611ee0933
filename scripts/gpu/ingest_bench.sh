# device CSV tests + 1-GPU bench (headline + ingest with first/warm loads); logs go to $LOGS
set -o pipefail
LOGS=${LOGS:-logs}
mkdir -p "$LOGS"
timeout -k 10 300 python -u -m pytest tests/test_csv_device.py tests/test_records.py -m gpu -x -q --timeout 120 --timeout-method thread > "$LOGS/ingest_tests.log" 2>&1 &&
timeout -k 10 300 python -u bench.py --full > "$LOGS/ingest_bench.log" 2>&1
