#!/usr/bin/env python3
"""Isolation forest on one GPU: whole ``IsolationForest.fit`` and ``score_samples`` calls of
``engine="philox"`` (models/iforest.py, csrc/kernels/iforest.hip) against ``engine="torch"`` (the
batched-tensor forest of models/outlier.py, the path these kernels stand beside) on the same card,
and scikit-learn's IsolationForest on the host for context.

* Standard normal rows with 1 % planted outliers, T = 100 trees, psi = 256, D = 4 and 16,
  n = 2^16, 2^20 and 2^24 (``--sizes``), ``contamination="auto"``.
* ``fit``: the torch engine always scores the training set, the philox engine does not when the
  contamination is ``auto``; ``fit_scored`` is the philox fit plus one ``score_samples`` of the
  training set, the like-for-like figure.
* ``--twin-sizes``: log2 n at which the twin on a host copy (``use_kernel=False``, what a dispatch
  cap would fall back to) is timed against the kernels as well.

Every time is a whole call ending in a device synchronise.  The two engines are timed in alternating
pairs after one warm-up each, medians of ``--repeats`` runs; a baseline whose warm-up took longer
than ``--slow`` seconds is timed twice, one that took longer than ``--very-slow`` seconds is not run
again (``*_runs`` says how many runs a figure rests on).  scikit-learn is timed once per size up to
``--sklearn-max`` (log2 n).  One JSON line per measurement, printed and appended to ``--out``."""
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

T, PSI = 100, 256


def data(n, D, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.randn((n, D), generator=g, device="cuda")
    k = max(1, n // 100)
    X[:k] += (torch.randint(0, 2, (k, D), generator=g, device="cuda").float() * 2 - 1) * 6
    return X


def timed(fn):
    torch.cuda.synchronize()
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


def measure(n, D, args, with_twin, with_sklearn):
    from avenir_amd.models.outlier import IsolationForest
    X = data(n, D)
    row = {"bench": "iforest", "n": n, "D": D, "trees": T, "psi": PSI}
    med = statistics.median
    new = lambda **kw: IsolationForest(n_estimators=T, max_samples=PSI, seed=1, engine="philox", **kw)
    old = lambda: IsolationForest(n_estimators=T, max_samples=PSI, seed=1)

    def fit_scored():
        m = new().fit(X)
        m.score_samples(X)
        return m

    ta, tb, mp, mt = pair(fit_scored, lambda: old().fit(X), args.repeats, args.slow, args.very_slow)
    row.update(philox_fit_scored_s=med(ta), philox_fit_scored_s_all=ta, torch_fit_s=med(tb), torch_fit_s_all=tb,
               torch_fit_runs=len(tb))
    row["torch_over_philox_fit_scored"] = row["torch_fit_s"] / row["philox_fit_scored_s"]
    tf = [timed(lambda: new().fit(X))[0] for _ in range(args.repeats + 1)][1:]
    row.update(philox_fit_s=med(tf), philox_fit_s_all=tf)
    ta, tb, sp, st = pair(lambda: mp.score_samples(X), lambda: mt.score_samples(X), args.repeats, args.slow, args.very_slow)
    row.update(philox_score_s=med(ta), philox_score_s_all=ta, torch_score_s=med(tb), torch_score_s_all=tb,
               torch_score_runs=len(tb), score_corr=float(torch.corrcoef(torch.stack([sp, st]))[0, 1]))
    row["torch_over_philox_score"] = row["torch_score_s"] / row["philox_score_s"]
    row["philox_score_rows_per_s"] = n / row["philox_score_s"]
    del st
    if with_twin:
        twin = lambda: new(use_kernel=False).fit(X)
        ta, tb, mk, mw = pair(lambda: new().fit(X), twin, args.repeats, args.slow, args.very_slow)
        row.update(philox_fit_s_vs_twin=med(ta), twin_on_host_fit_s=med(tb), twin_on_host_fit_runs=len(tb),
                   twin_bits_equal=bool(torch.equal(mk.feat, mw.feat) and torch.equal(mk.size, mw.size) and
                                        torch.equal(mk.thr.view(torch.int32), mw.thr.view(torch.int32))))
        ta, tb, sk_, sw = pair(lambda: mk.path_length(X), lambda: mw.path_length(X), args.repeats, args.slow, args.very_slow)
        row.update(philox_path_s_vs_twin=med(ta), twin_on_host_path_s=med(tb), twin_on_host_path_runs=len(tb),
                   twin_path_bits_equal=bool(torch.equal(sk_.view(torch.int32), sw.view(torch.int32))))
        row["kernel_wins"] = bool(row["philox_fit_s_vs_twin"] < row["twin_on_host_fit_s"] and
                                  row["philox_path_s_vs_twin"] < row["twin_on_host_path_s"])
    if with_sklearn:
        from sklearn.ensemble import IsolationForest as SK
        Xh = X.cpu().numpy()
        t0 = time.perf_counter()
        sk = SK(n_estimators=T, max_samples=PSI, random_state=0).fit(Xh)
        t1 = time.perf_counter()
        ss = sk.score_samples(Xh)
        t2 = time.perf_counter()
        row.update(sklearn_fit_s=t1 - t0, sklearn_score_s=t2 - t1, sklearn_runs=1,
                   sklearn_score_corr=float(np.corrcoef(ss, sp.cpu().numpy())[0, 1]))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iforest_bench.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slow", type=float, default=2.0)
    ap.add_argument("--very-slow", type=float, default=20.0)
    ap.add_argument("--dims", type=int, nargs="*", default=[4, 16])
    ap.add_argument("--sizes", type=int, nargs="*", default=[16, 20, 24], help="log2 n")
    ap.add_argument("--twin-sizes", type=int, nargs="*", default=[8, 12, 16], help="log2 n also timed against the twin")
    ap.add_argument("--sklearn-max", type=int, default=20, help="largest log2 n scikit-learn is run at")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_iforest needs a GPU")
    for lg in sorted(set(args.sizes) | set(args.twin_sizes)):
        for D in args.dims:
            row = measure(1 << lg, D, args, lg in args.twin_sizes, lg <= args.sklearn_max)
            print(json.dumps(row), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
