#!/usr/bin/env python3
"""Many k-means fits on one GPU: ``KMeans.fit_many`` through the device Lloyd loops
(models/kmeans_groups.py, csrc/kernels/kmeans_groups.hip: one workgroup per (group, k, restart)
run, one launch for the whole call) against the per-model loop of ``KMeans.fit`` (the same call
under ``AVMI_KMEANS_GROUPS=0``: three launches and one host read per iteration and launch group).

Two shapes, ks [2, 3, 4], 3 restarts, 10 iterations, 3 blobs per group:
  * 7 groups x 68 k rows x 2 dims (the kMeansPlusPlusCluster job at 480 k lines);
  * 4,096 groups x 120 rows x 2 dims (one model per customer or device key).

The two paths alternate in one process, ``--repeats`` synchronised pairs after a warm-up of each,
with the same data and the same initial centroids; one JSON line per path and shape (median, min,
max, all times) and one with the ratios (of the medians, and the smallest of any pair), printed and
written to ``--out``."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS, RESTARTS, ITERS = [2, 3, 4], 3, 10
SHAPES = [(7, 68_000, 2), (4096, 120, 2)]


def make_groups(groups: int, rows: int, dims: int, device) -> list[torch.Tensor]:
    g = torch.Generator().manual_seed(groups * 1000 + rows)
    c = torch.randint(0, 3, (groups, rows, 1), generator=g).float()
    X = c * torch.tensor([4.0, 3.0] * (dims // 2 + 1))[:dims] + 0.3 * torch.randn((groups, rows, dims), generator=g)
    return list(X.to(device).unbind(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "kmeans_groups_bench.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--loop-groups", type=int, default=0,
                    help="time the per-model loop on the first N groups only and scale it up (0: all groups)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kmeans_groups needs a GPU")
    from avenir_amd.models.cluster import KMeans
    dev = torch.device("cuda")
    rows_out = []

    def emit(row):
        rows_out.append(row)
        print(json.dumps(row), flush=True)

    for groups, rows, dims in SHAPES:
        Xs = make_groups(groups, rows, dims, dev)
        models = [KMeans(KS, n_init=RESTARTS, max_iter=ITERS) for _ in Xs]
        inits = KMeans.init_many(models, Xs)
        nl = groups if not args.loop_groups else min(groups, args.loop_groups)

        def run(batched: bool) -> float:
            os.environ["AVMI_KMEANS_GROUPS"] = "1" if batched else "0"
            n = groups if batched else nl
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            KMeans.fit_many(models[:n], Xs[:n], inits[:n])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * (1.0 if batched else groups / nl)

        run(True)
        run(False)                                  # warm-up of both
        tb, tl = [], []
        for _ in range(args.repeats):               # alternating pairs
            tl.append(run(False))
            tb.append(run(True))
        os.environ.pop("AVMI_KMEANS_GROUPS", None)
        base = {"bench": "kmeans_groups", "groups": groups, "rows_per_group": rows, "dims": dims, "ks": KS,
                "restarts": RESTARTS, "max_iter": ITERS, "runs": groups * len(KS) * RESTARTS}
        for impl, ts in (("fit_many_batched", tb), ("per_model_loop", tl)):
            emit({**base, "impl": impl, "median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts),
                  "all_s": ts, **({"loop_groups_timed": nl} if impl == "per_model_loop" else {})})
        emit({**base, "impl": "ratio", "loop_over_batched_median": statistics.median(tl) / statistics.median(tb),
              "loop_over_batched_min_pair": min(a / b for a, b in zip(tl, tb)),
              "batched_faster_in_every_pair": all(a > b for a, b in zip(tl, tb))})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for row in rows_out:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
