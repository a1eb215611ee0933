#!/usr/bin/env python3
"""Agglomerative clustering on one GPU: whole ``AgglomerativeClustering.fit`` calls on the device
kernels (models/agglo.py, csrc/kernels/agglo.hip) against scikit-learn's AgglomerativeClustering on
the host, and against the numpy twin on a host copy (``use_kernel=False``), which is the path a
dispatch cap would fall back to.

* Gaussian blobs (8 centres, unit variance), D = 8, n = 2^10, 2^12, 2^13 and 2^14, all four linkages
  with the euclidean metric, n_clusters = 8.
* ``--twin-sizes``: log2 n at which the twin-on-host path is timed against the kernels as well (the
  small sizes are where per-round launches and the one counter read per round could lose).

Every time is a whole fit ending in a device synchronise.  The kernel path and a baseline are timed
in alternating pairs after one warm-up each, medians of ``--repeats`` runs; a baseline whose warm-up
took longer than ``--slow`` seconds is timed twice, one that took longer than ``--very-slow`` seconds
is not run again (its warm-up time is recorded, ``*_runs`` says how many runs a figure rests on).
``rounds`` is the number of reciprocal-pair rounds of the fit.  One JSON line per measurement,
printed and appended to ``--out``."""
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

LINKAGES = ["single", "complete", "average", "ward"]
K = 8


def blobs(n, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn((8, D), generator=g) * 12
    return (centres[torch.randint(0, 8, (n,), generator=g)] + torch.randn((n, D), generator=g)).float()


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
    pairs = np.unique(np.stack([np.asarray(a), np.asarray(b)], 1), axis=0)
    return bool(len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1])))


def measure(n, D, link, args, with_twin):
    from sklearn.cluster import AgglomerativeClustering as SkAgglomerative
    from avenir_amd.models.agglo import AgglomerativeClustering
    Xh = blobs(n, D)
    X, Xd = Xh.cuda(), Xh.double().numpy()
    fit = lambda: AgglomerativeClustering(n_clusters=K, linkage=link).fit(X)
    row = {"bench": "agglo", "n": n, "D": D, "linkage": link, "metric": "euclidean", "n_clusters": K}
    sk = lambda: SkAgglomerative(n_clusters=K, linkage=link).fit(Xd)
    ta, tb, m, skm = pair(fit, sk, args.repeats, args.slow, args.very_slow)
    row.update(rounds=m.rounds_, kernel_fit_s=statistics.median(ta), kernel_fit_s_all=ta, sklearn_s=statistics.median(tb),
               sklearn_s_all=tb, sklearn_runs=len(tb), sklearn_same_partition=same_partition(m.labels_.cpu(), skm.labels_))
    row["sklearn_over_kernel"] = row["sklearn_s"] / row["kernel_fit_s"]
    if with_twin:
        twin = lambda: AgglomerativeClustering(n_clusters=K, linkage=link, use_kernel=False).fit(X)
        ta, tb, m, tw = pair(fit, twin, args.repeats, args.slow, args.very_slow)
        row.update(kernel_fit_s_vs_twin=statistics.median(ta), twin_on_host_s=statistics.median(tb), twin_on_host_s_all=tb,
                   twin_on_host_runs=len(tb), twin_bits_equal=bool(
                       torch.equal(m.children_, tw.children_) and torch.equal(m.labels_, tw.labels_) and
                       torch.equal(m.distances_.view(torch.int32), tw.distances_.view(torch.int32))))
        row["twin_over_kernel"] = row["twin_on_host_s"] / row["kernel_fit_s_vs_twin"]
        row["kernel_wins"] = bool(row["kernel_fit_s_vs_twin"] < row["twin_on_host_s"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agglo_bench.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slow", type=float, default=1.0)
    ap.add_argument("--very-slow", type=float, default=8.0)
    ap.add_argument("--dim", type=int, default=8)
    ap.add_argument("--sizes", type=int, nargs="*", default=[10, 12, 13, 14], help="log2 n")
    ap.add_argument("--twin-sizes", type=int, nargs="*", default=[5, 7, 10, 12], help="log2 n also timed against the twin")
    ap.add_argument("--linkages", nargs="*", default=LINKAGES)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_agglo needs a GPU")
    for lg in sorted(set(args.sizes) | set(args.twin_sizes)):
        for link in args.linkages:
            row = measure(1 << lg, args.dim, link, args, lg in args.twin_sizes)
            print(json.dumps(row), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
