# ingest refresh after the upload changes: record tests, bench.py, text-layout tokenize + job rates;
# logs go to $LOGS
set -o pipefail
LOGS=${LOGS:-logs}
mkdir -p "$LOGS"
timeout -k 10 300 python -u -m pytest tests/test_csv_device.py tests/test_records.py tests/test_native_jobs.py -m gpu -x -q --timeout 120 --timeout-method thread > "$LOGS/ir_tests.log" 2>&1 &&
timeout -k 10 300 python -u bench.py --full > "$LOGS/ir_bench.log" 2>&1 &&
timeout -k 10 600 python -u benchmarks/bench_ingest.py --jobs --out "$LOGS/ir_ingest.jsonl" > "$LOGS/ir_ingest.log" 2>&1
