#!/usr/bin/env python3
"""Tabu search over an assignment domain on one GPU: the one-launch kernel (optimize/tabu.py,
csrc/kernels/optim.hip::tabu_assign_kernel) against the generic torch path
(TabuSearch(use_kernel=False): about twenty launches and five host reads per iteration).

* a synthetic 24 x 10 assignment with a 15 % conflict density (the instance of
  tests/test_tabu_assign.py) at 16, 1,024 and 16,384 chains;
* ``--sweep``: 16 chains over growing L x V up to the kernel's LDS limit (one chain is one wave, so
  its time grows with L V / 64 whatever the chain count) -> ``--sweep-out``.

200 iterations, tenure 7.  Every time is a whole ``TabuSearch.run()`` on CUDA (start solutions,
pricing, launches, download), the two implementations timed in alternating pairs after one warm-up
each, medians of ``--repeats`` runs.  ``kernel_wins`` applies the rule of the default dispatch: the
kernel's median is below the generic path's.  One JSON line per measurement, printed and appended
to ``--out``."""
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

ITERS, TENURE = 200, 7
SWEEP = ((24, 10), (48, 10), (64, 16), (96, 20), (128, 24), (128, 40), (160, 48), (100, 100))


def _random_assignment(L, V, seed, density, dev):
    from avenir_amd.optimize.domain import AssignmentDomain
    g = torch.Generator().manual_seed(seed)
    cost = torch.rand((L, V), generator=g) * 100
    conf = torch.rand((L, L), generator=g) < density
    return AssignmentDomain(cost, conf | conf.T, invalid_cost=1e3).to(dev)


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


def _tabu_pair(d, chains: int, repeats: int) -> dict:
    from avenir_amd.optimize.search import TabuSearch
    from avenir_amd.optimize.tabu import tabu_assign_plan
    kw = dict(n_chains=chains, iters=ITERS, tenure=TENURE, seed=1)
    res = {}
    ker = lambda: res.__setitem__("k", TabuSearch(d, use_kernel=True, **kw).run())
    gen = lambda: res.__setitem__("t", TabuSearch(d, use_kernel=False, **kw).run())
    k_s, t_s, ks, ts = _pairs(ker, gen, repeats)
    assert res["k"].stats["engine"] == "tabu_assign_kernel" and "engine" not in res["t"].stats
    waves, staged, lds = tabu_assign_plan(d.L, d.V)
    return {"L": d.L, "V": d.V, "cells": d.L * d.V, "chains": chains, "iters": ITERS, "tenure": TENURE,
            "waves_per_workgroup": waves, "tables_in_lds": staged, "lds_bytes": lds,
            "kernel_run_s": k_s, "torch_run_s": t_s, "kernel_run_s_all": ks, "torch_run_s_all": ts,
            "torch_over_kernel": t_s / k_s, "kernel_wins": bool(k_s < t_s),
            "chain_iters_per_s_kernel": chains * ITERS / k_s, "kernel_best_cost": float(res["k"].best_cost),
            "torch_best_cost": float(res["t"].best_cost)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tabu_assign_bench.jsonl"))
    ap.add_argument("--sweep-out", default=os.path.join(ROOT, "profiles", "tabu_assign_cap_sweep.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--chains", type=int, nargs="*", default=[16, 1024, 16384])
    ap.add_argument("--sweep", action="store_true", help="also run the 16-chain size sweep")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tabu_assign needs a GPU")
    from avenir_amd.optimize.tabu import LDS_LIMIT, tabu_assign_lds
    dev = torch.device("cuda")

    def emit(path, row):
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as fh:
            fh.write(json.dumps(row) + "\n")

    d = _random_assignment(24, 10, 1, 0.15, dev)
    for chains in args.chains:
        emit(args.out, {"bench": "tabu_assign", "density": 0.15, **_tabu_pair(d, chains, args.repeats)})
    if args.sweep:
        for L, V in SWEEP:
            assert tabu_assign_lds(L, V) <= LDS_LIMIT, (L, V)
            d = _random_assignment(L, V, 1, 0.15, dev)
            emit(args.sweep_out, {"bench": "tabu_assign_cap_sweep", "density": 0.15,
                                  **_tabu_pair(d, 16, args.repeats)})


if __name__ == "__main__":
    main()
