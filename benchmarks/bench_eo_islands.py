#!/usr/bin/env python3
"""The evolutionary optimiser on one GPU: the one-launch island kernels (optimize/eo.py,
csrc/kernels/optim.hip::eo_assign_kernel, eo_meeting_kernel and eo_subset_kernel) against the torch path
(EvolutionaryOptimizer(use_kernel=False): about 15 small launches and a host read per iteration,
whatever the island count).

* assign: the 24 x 10 assignment at 15 % conflicts (tests/_eo.py) at 1, 64 and 4,096 islands;
* meeting: the reference configuration of bench_ga_meeting.py (10 meetings, 20 people) at 1, 64 and
  4,096 islands;
* subset: the churn naive-Bayes model of bench_ga_subset.py (5 features, 2 classes) at N = 4,000 and
  N = 65,536 rows, at 1, 64 and 1,024 islands;

300 iterations, pool 5, select 3, purge weight 0.7, age scale 1: the reference's defaults.  Every time
is a whole ``EvolutionaryOptimizer.run()`` on CUDA (start pools, pricing, launch, download), the two
implementations timed in alternating pairs after one warm-up each, medians of ``--repeats`` runs.
``kernel_wins`` applies the rule of the default dispatch: the kernel's median is below the torch
path's by more than the larger of the two min-max spreads.  The kernels alone and multi-GPU runs are
not measured here.  ``--sweep`` adds subset runs at N = 2^12 .. 2^20 rows and 1 island (``--sweep-out``).
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

ITERS, POOL, SELECT = 300, 5, 3


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


def _assignment(dev):
    from avenir_amd.optimize import AssignmentDomain
    g = torch.Generator().manual_seed(0)
    cost = torch.rand((24, 10), generator=g) * 100
    conf = torch.rand((24, 24), generator=g) < 0.15
    return AssignmentDomain(cost, conf | conf.T, invalid_cost=1e3).to(dev)


def _subset_domain(n: int, dev):
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


def _eo_pair(d, engine: str, islands: int, repeats: int) -> dict:
    from avenir_amd.optimize.search import EvolutionaryOptimizer
    kw = dict(islands=islands, pool=POOL, select=SELECT, iters=ITERS, seed=1)
    res = {}
    ker = lambda: res.__setitem__("k", EvolutionaryOptimizer(d, use_kernel=True, **kw).run())
    gen = lambda: res.__setitem__("t", EvolutionaryOptimizer(d, use_kernel=False, **kw).run())
    k_s, t_s, ks, ts = _pairs(ker, gen, repeats)
    assert res["k"].stats["engine"] == engine and "engine" not in res["t"].stats
    spread = max(max(ks) - min(ks), max(ts) - min(ts))
    return {"islands": islands, "iters": ITERS, "pool": POOL, "select": SELECT,
            "kernel_run_s": k_s, "torch_run_s": t_s, "kernel_run_s_all": ks, "torch_run_s_all": ts,
            "torch_over_kernel": t_s / k_s, "larger_spread_s": spread, "kernel_wins": bool(k_s < t_s - spread),
            "island_iters_per_s_kernel": islands * ITERS / k_s, "kernel_best_cost": float(res["k"].best_cost),
            "torch_best_cost": float(res["t"].best_cost)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eo_islands_bench.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--assign-islands", type=int, nargs="*", default=[1, 64, 4096])
    ap.add_argument("--meeting-islands", type=int, nargs="*", default=[1, 64, 4096])
    ap.add_argument("--rows", type=int, nargs="*", default=[4000, 65536])
    ap.add_argument("--subset-islands", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--sweep", action="store_true", help="also run the one-island row sweep")
    ap.add_argument("--sweep-out", default=os.path.join(ROOT, "profiles", "eo_subset_cap_sweep.jsonl"))
    ap.add_argument("--sweep-repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eo_islands needs a GPU")
    from avenir_amd.optimize.domains import MeetingScheduleDomain
    dev = torch.device("cuda")

    def emit(path, row):
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as fh:
            fh.write(json.dumps(row) + "\n")

    d = _assignment(dev)
    for islands in args.assign_islands:
        emit(args.out, {"bench": "eo_islands", "domain": "assign", "positions": 24, "values": 10,
                        **_eo_pair(d, "eo_assign_kernel", islands, args.repeats)})
    d = MeetingScheduleDomain.random_instance(10, 20, seed=3, device=dev)
    for islands in args.meeting_islands:
        emit(args.out, {"bench": "eo_islands", "domain": "meeting", "meetings": 10, "people": 20,
                        **_eo_pair(d, "eo_meeting_kernel", islands, args.repeats)})
    for n in args.rows:
        d = _subset_domain(n, dev)
        for islands in args.subset_islands:
            emit(args.out, {"bench": "eo_islands", "domain": "subset", "rows": n, "features": d.F,
                            "classes": int(d.loglik.shape[2]),
                            **_eo_pair(d, "eo_subset_kernel", islands, args.repeats)})
    if args.sweep:
        for e in range(12, 21):
            d = _subset_domain(1 << e, dev)
            emit(args.sweep_out, {"bench": "eo_subset_cap_sweep", "domain": "subset", "rows": 1 << e, "features": d.F,
                                  "classes": int(d.loglik.shape[2]),
                                  **_eo_pair(d, "eo_subset_kernel", 1, args.sweep_repeats)})


if __name__ == "__main__":
    main()
