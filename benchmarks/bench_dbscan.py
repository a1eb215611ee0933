#!/usr/bin/env python3
"""DBSCAN on one GPU: whole ``DBSCAN.fit`` calls on the device kernels (models/dbscan.py,
csrc/kernels/dbscan.hip) against ``cluster.dbscan`` (torch.cdist blocks and label propagation) on
the same device and against sklearn's DBSCAN on the host.

* Gaussian blobs (8 centres, unit variance) in D = 2, 8 and 16; n = 2^12, 2^14 and 2^16 against
  both baselines, n = 2^17 and 2^18 for the kernel path alone.  eps is the median distance of 512
  sampled points to their 20th neighbour, so a point has roughly 10 to 30 neighbours;
  min_samples = 10.
* one dense setting (D = 2, n = 2^16, eps = 1): every point of a blob has thousands of neighbours.

Every time is a whole fit ending in a device synchronise.  The kernel path and a baseline are timed
in alternating pairs after one warm-up each, medians of ``--repeats`` runs; a baseline whose warm-up
took longer than ``--slow`` seconds is timed twice, one that took longer than ``--very-slow``
seconds is not run again (its warm-up time is recorded, ``*_runs`` says how many runs a figure
rests on).  ``kernel_wins`` applies the rule of the default dispatch.  One JSON line per
measurement, printed and appended to ``--out``.

``--profile N D`` runs three warmed fits of one shape and nothing else: the run to put under
``rocprofv3 --kernel-trace --stats`` for the per-kernel times."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIN_SAMPLES = 10


def blobs(n, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn((8, D), generator=g) * 12
    return (centres[torch.randint(0, 8, (n,), generator=g)] + torch.randn((n, D), generator=g)).float()


def sparse_eps(X):
    from avenir_amd.ops import distance as dist
    d, _ = dist.knn(X[:512], X, 21)
    return float(d[:, 20].median())


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def pair(fa, fb, repeats, slow, very_slow):
    """(times of a, times of b, last results): alternating runs after one warm-up each."""
    wa, ra = timed(fa)
    wb, rb = timed(fb)
    nb = repeats if wb <= slow else 2 if wb <= very_slow else 0
    ta, tb = [], []
    for r in range(repeats):
        ta.append(timed(fa)[0])
        if r < nb:
            tb.append(timed(fb)[0])
    return ta, tb or [wb], ra, rb


def same_partition(a, b):
    """Equal up to the numbering of the clusters (noise = -1 on both sides)."""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a < 0, b < 0):
        return False
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


def measure(n, D, eps, tag, args, baselines):
    from sklearn.cluster import DBSCAN as SkDBSCAN
    from avenir_amd.models import cluster
    from avenir_amd.models.dbscan import DBSCAN
    Xh = blobs(n, D)
    X = Xh.cuda()
    if eps is None:
        eps = sparse_eps(X)
    fit = lambda: DBSCAN(eps, MIN_SAMPLES).fit(X)
    row = {"bench": "dbscan", "setting": tag, "n": n, "D": D, "eps": eps, "min_samples": MIN_SAMPLES}
    if baselines:
        ta, tb, m, lab = pair(fit, lambda: cluster.dbscan(X, eps, MIN_SAMPLES), args.repeats, args.slow, args.very_slow)
        row.update(kernel_fit_s=statistics.median(ta), kernel_fit_s_all=ta, torch_dbscan_s=statistics.median(tb),
                   torch_dbscan_s_all=tb, torch_dbscan_runs=len(tb),
                   torch_same_partition=same_partition(m.labels_.cpu(), lab.cpu()))
        row["torch_over_kernel"] = row["torch_dbscan_s"] / row["kernel_fit_s"]
        row["kernel_wins"] = bool(row["kernel_fit_s"] < row["torch_dbscan_s"])
        Xd = Xh.double().numpy()
        sk = lambda: SkDBSCAN(eps=eps, min_samples=MIN_SAMPLES).fit(Xd)
        ta, tb, m, skm = pair(fit, sk, args.repeats, args.slow, args.very_slow)
        row.update(kernel_fit_s_vs_sklearn=statistics.median(ta), sklearn_s=statistics.median(tb), sklearn_s_all=tb,
                   sklearn_runs=len(tb), sklearn_labels_equal=bool(np.array_equal(m.labels_.cpu().numpy(), skm.labels_)))
        row["sklearn_over_kernel"] = row["sklearn_s"] / row["kernel_fit_s_vs_sklearn"]
    else:
        timed(fit)
        ta = [timed(fit)[0] for _ in range(args.repeats)]
        m = fit()
        row.update(kernel_fit_s=statistics.median(ta), kernel_fit_s_all=ta)
    row.update(mean_neighbours=float(m.counts_.float().mean()) - 1, core_points=int(m.core_sample_indices_.numel()),
               clusters=m.n_clusters_, noise=int((m.labels_ < 0).sum()),
               pairs_per_s_three_sweeps=3.0 * n * n / row["kernel_fit_s"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbscan_bench.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slow", type=float, default=1.0)
    ap.add_argument("--very-slow", type=float, default=8.0)
    ap.add_argument("--dims", type=int, nargs="*", default=[2, 8, 16])
    ap.add_argument("--sizes", type=int, nargs="*", default=[12, 14, 16], help="log2 n against the baselines")
    ap.add_argument("--kernel-sizes", type=int, nargs="*", default=[17, 18], help="log2 n for the kernel path alone")
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--profile", type=int, nargs=2, metavar=("N", "D"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dbscan needs a GPU")
    if args.profile:
        from avenir_amd.models.dbscan import DBSCAN
        X = blobs(*args.profile).cuda()
        eps = sparse_eps(X)
        for _ in range(4):
            m = DBSCAN(eps, MIN_SAMPLES).fit(X)
        torch.cuda.synchronize()
        print(json.dumps({"profile": args.profile, "eps": eps, "clusters": m.n_clusters_}))
        return

    def emit(row):
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")

    for D in args.dims:
        for lg in args.sizes:
            emit(measure(1 << lg, D, None, "sparse", args, True))
        for lg in args.kernel_sizes:
            emit(measure(1 << lg, D, None, "sparse", args, False))
    if not args.no_dense:
        emit(measure(1 << 16, 2, 1.0, "dense", args, True))


if __name__ == "__main__":
    main()
