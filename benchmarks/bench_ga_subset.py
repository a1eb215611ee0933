#!/usr/bin/env python3
"""Island GA over feature subsets scored by naive Bayes on one GPU: the one-launch island kernel
(optimize/ga_subset.py, csrc/kernels/optim.hip::ga_subset_kernel) against the per-island torch path
(GeneticAlgorithm(use_kernel=False): about a dozen small launches per island and generation plus one
[children, F] x [F, N C] GEMM).

The domain is the churn naive-Bayes model (5 features, 2 classes) at N = 4,000 and N = 65,536 rows,
pool 30, mating 10, replacement 10, 100 generations, at 1, 64 and 256 islands.  Every time is a whole
``GeneticAlgorithm.run()`` on CUDA (initial pools, pricing, launches, download), the two
implementations timed in alternating pairs after one warm-up each, medians of ``--repeats`` runs.
``scoring`` rows time one ``FeatureSubsetDomain.errors`` call (subset_errors_kernel) on 1,024 masks
against ``domain.cost`` on the same masks.  ``--sweep`` adds the row-cap sweep (N = 2^12 .. 2^20 at 1
and 64 islands) written to ``--sweep-out``; the engine's row cap is lifted for the whole benchmark.
One JSON line per measurement, printed and appended to ``--out``."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P, MATING, R, G = 30, 10, 10, 100


def _pairs(fa, fb, repeats: int):
    """Alternating a / b runs after one warm-up each -> (median a, median b, all a, all b)."""
    fa()
    fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(repeats):
        for fn, ts in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
    return statistics.median(ta), statistics.median(tb), ta, tb


def _domain(n: int, dev):
    from avenir_amd.data.synth import CHURN_SCHEMA, churn_device
    from avenir_amd.data.table import Table
    from avenir_amd.models.bayes import NaiveBayes
    from avenir_amd.optimize.domains import FeatureSubsetDomain
    from avenir_amd.utils.schema import FeatureSchema
    schema = FeatureSchema.from_json(CHURN_SCHEMA)
    codes, labels = churn_device(n, seed=0, device=dev)
    t = Table(schema, n, codes, schema.feature_fields, torch.zeros((0, codes.shape[1]), device=dev), [], labels,
              schema.find_class_attr_field())
    nb = NaiveBayes(schema).fit(t)
    return FeatureSubsetDomain.from_naive_bayes(nb, t, t.labels[:n], min_size=1)


def _ga_pair(d, islands: int, generations: int, repeats: int) -> dict:
    from avenir_amd.optimize.search import GeneticAlgorithm
    kw = dict(islands=islands, pool=P, mating=MATING, replacement=R, generations=generations, seed=1)
    res = {}
    ker = lambda: res.__setitem__("k", GeneticAlgorithm(d, use_kernel=True, **kw).run())
    gen = lambda: res.__setitem__("t", GeneticAlgorithm(d, use_kernel=False, **kw).run())
    k_s, t_s, ks, ts = _pairs(ker, gen, repeats)
    assert res["k"].stats["engine"] == "ga_subset_kernel" and "engine" not in res["t"].stats
    N, F, C = d.loglik.shape
    return {"rows": N, "features": F, "classes": C, "islands": islands, "pool": P, "mating": MATING, "replacement": R,
            "generations": generations, "kernel_run_s": k_s, "torch_run_s": t_s, "kernel_run_s_all": ks,
            "torch_run_s_all": ts, "torch_over_kernel": t_s / k_s, "kernel_best_cost": float(res["k"].best_cost),
            "torch_best_cost": float(res["t"].best_cost)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ga_subset_bench.jsonl"))
    ap.add_argument("--sweep-out", default=os.path.join(ROOT, "profiles", "ga_subset_cap_sweep.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="*", default=[4000, 65536])
    ap.add_argument("--islands", type=int, nargs="*", default=[1, 64, 256])
    ap.add_argument("--sweep", action="store_true", help="also run the row-cap sweep")
    ap.add_argument("--sweep-islands", type=int, nargs="*", default=[1, 64])
    ap.add_argument("--sweep-repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ga_subset needs a GPU")
    from avenir_amd.optimize import ga_subset
    dev = torch.device("cuda")

    def emit(path, row):
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as fh:
            fh.write(json.dumps(row) + "\n")

    cap = ga_subset.ROW_CAP
    ga_subset.ROW_CAP = 1 << 30          # both engines are timed at every size: the engine's row cap is lifted
    try:
        for n in args.rows:
            d = _domain(n, dev)
            for islands in args.islands:
                emit(args.out, {"bench": "ga_subset", "row_cap": cap, **_ga_pair(d, islands, G, args.repeats)})
            g = torch.Generator(device=dev).manual_seed(2)
            sol = torch.randint(0, 2, (1024, d.F), generator=g, device=dev)
            out = {}
            e_s, c_s, es, cs = _pairs(lambda: out.__setitem__("e", d.errors(sol)),
                                      lambda: out.__setitem__("c", d.cost(sol)), args.repeats)
            differ = int((out["e"].float() / n != out["c"]).sum())
            emit(args.out, {"bench": "ga_subset", "impl": "scoring", "rows": n, "features": d.F, "masks": 1024,
                            "errors_call_s": e_s, "cost_call_s": c_s, "errors_call_s_all": es, "cost_call_s_all": cs,
                            "cost_over_errors": c_s / e_s, "masks_where_gemm_cost_differs": differ})
        if args.sweep:                   # the sweep is what sets the cap
            for e in range(12, 21):
                d = _domain(1 << e, dev)
                for islands in args.sweep_islands:
                    emit(args.sweep_out, {"bench": "ga_subset_cap_sweep", "row_cap": cap,
                                          **_ga_pair(d, islands, G, args.sweep_repeats)})
    finally:
        ga_subset.ROW_CAP = cap


if __name__ == "__main__":
    main()
