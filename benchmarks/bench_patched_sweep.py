#!/usr/bin/env python3
"""Where the patched record stream stops paying: the K2 class histogram over churn-shaped records
with a controlled share of escaped records, patched (10 bits + 2 bytes per exception) against the
plain 11-bit mixed-radix stream (``AVMI_ROWPACK_KERNEL=radix``) in one process.

The churn generator never emits acctAge = "1", so a state with that digit has count 0 in a sample of
clean records and the 57 highest-coded of those states rank past the 1023 cells a 10-bit record
stores.  A share s of the records is overwritten with states drawn uniformly from those 57; the
states are ranked from clean records only (``attach_patched(sample=...)``) and the width is forced
to 10, so the overwritten records escape (with the records of the few rare states a 2^20-record
sample misses, about 1e-5 of all; the line reports the exact count).

Per share: 5 warm-up calls, then device events around 20 calls, for each stream in turn,
``--repeats`` times.  One JSON line per share, printed and appended to ``--out``: the times of every
repetition, the bytes each kernel reads, their ratio, and whether patched won every repetition.  The
dispatch margin ``PATCH_MARGIN`` (ops/histogram.py) is read from this file."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHARES = [0.0, 0.005, 0.01, 0.02, 0.04, 0.08]
CHURN = [4, 3, 3, 3, 5]
ESCAPING = (159, 216)      # codes of the zero-count states ranked 1023 and later (class digit first)


def records(n: int, share: float, dev):
    from avenir_amd.data.synth import churn_device
    codes, labels = churn_device(n, seed=4321, device=dev)
    g = torch.Generator(device=dev).manual_seed(7)
    hit = torch.rand(n, generator=g, device=dev) < share
    state = torch.randint(ESCAPING[0], ESCAPING[1], (n,), generator=g, device=dev)
    labels[:n] = torch.where(hit, (state % 2).to(torch.uint8), labels[:n])
    rest = state // 2
    for k, r in enumerate(CHURN):
        codes[k, :n] = torch.where(hit, (rest % r).to(torch.uint8), codes[k, :n])
        rest = rest // r
    return codes, labels, hit


def time_calls(fn, calls: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 28)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patched_cap_sweep.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_patched_sweep: no GPU", file=sys.stderr)
        return 1
    from avenir_amd.ops import histogram as H

    dev = torch.device("cuda:0")
    n = args.rows
    for share in SHARES:
        codes, labels, hit = records(n, share, dev)
        rp = H.pack_rows(codes, n, CHURN, labels, 2)
        clean = (~hit).nonzero().flatten()
        H.attach_patched(rp, bits=10, sample=clean[::max(1, clean.numel() // H.PATCH_SAMPLE)])
        E = int(rp.exc_index.numel())
        assert rp.bits == 11 and rp.patched_bits == 10
        del codes, labels, hit, clean
        out = torch.zeros((2, sum(CHURN) + 1), dtype=torch.int64, device=dev)
        fn = lambda: H.class_histogram_packed(rp, out=out, count_labels=True)
        tables = {}
        times = {"patched": [], "radix": []}
        for _ in range(args.repeats):
            for kind in ("patched", "radix"):
                os.environ["AVMI_ROWPACK_KERNEL"] = "dense" if kind == "patched" else "radix"
                out.zero_()
                times[kind].append(time_calls(fn, args.calls, args.warmup))
                tables[kind] = (out // (args.calls + args.warmup)).cpu()
        os.environ.pop("AVMI_ROWPACK_KERNEL", None)
        assert torch.equal(tables["patched"], tables["radix"])
        groups = (n + 31) // 32
        pb, rb = 10 * groups * 4 + 2 * E, 11 * groups * 4
        line = {"bench": "patched_cap_sweep", "rows": n, "share": share, "exceptions": E,
                "patched_bytes": pb, "radix_bytes": rb, "byte_ratio": pb / rb,
                "patched_ms": times["patched"], "radix_ms": times["radix"],
                "patched_ms_median": statistics.median(times["patched"]),
                "radix_ms_median": statistics.median(times["radix"]),
                "patched_wins_every_repeat": max(times["patched"]) < min(times["radix"]),
                "calls": args.calls, "warmup": args.warmup}
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as fh:
            fh.write(json.dumps(line) + "\n")
        del rp, out
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
