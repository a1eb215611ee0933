#!/usr/bin/env python3
"""Simulated annealing over the meeting-schedule and feature-subset domains on one GPU: the
one-launch chain kernels (optimize/sa.py, csrc/kernels/optim.hip::sa_meeting_kernel and
sa_subset_kernel) against the generic torch path (SimulatedAnnealing(use_kernel=False): about a
dozen small launches and three host reads per move, whatever the chain count).

* meeting: the reference configuration of bench_ga_meeting.py (10 meetings, 20 people) at 1, 64 and
  4,096 chains;
* subset: the churn naive-Bayes model of bench_ga_subset.py (5 features, 2 classes) at N = 4,000 and
  N = 65,536 rows, at 1, 64 and 1,024 chains;

300 moves, geometric cooling 0.97 every 3 moves, 3 retries.  Every time is a whole
``SimulatedAnnealing.run()`` on CUDA (start solutions, pricing, launches, download), the two
implementations timed in alternating pairs after one warm-up each, medians of ``--repeats`` runs.
``kernel_wins`` applies the rule of the default dispatch: the kernel's median is below the generic
path's by more than the larger of the two min-max spreads.  ``--sweep`` adds subset runs at
N = 2^12 .. 2^20 rows and 1 chain (``--sweep-out``).  One JSON line per measurement, printed and
appended to ``--out``."""
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

MOVES, COOL, INTERVAL, RETRY = 300, 0.97, 3, 3


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


def _sa_pair(d, engine: str, chains: int, t0: float, repeats: int) -> dict:
    from avenir_amd.optimize.search import SimulatedAnnealing
    kw = dict(n_chains=chains, iters=MOVES, t0=t0, cooling=COOL, interval=INTERVAL, max_retry=RETRY, seed=1)
    res = {}
    ker = lambda: res.__setitem__("k", SimulatedAnnealing(d, use_kernel=True, **kw).run())
    gen = lambda: res.__setitem__("t", SimulatedAnnealing(d, use_kernel=False, **kw).run())
    k_s, t_s, ks, ts = _pairs(ker, gen, repeats)
    assert res["k"].stats["engine"] == engine and "engine" not in res["t"].stats
    spread = max(max(ks) - min(ks), max(ts) - min(ts))
    return {"chains": chains, "moves": MOVES, "t0": t0, "cooling": COOL, "interval": INTERVAL, "max_retry": RETRY,
            "kernel_run_s": k_s, "torch_run_s": t_s, "kernel_run_s_all": ks, "torch_run_s_all": ts,
            "torch_over_kernel": t_s / k_s, "larger_spread_s": spread, "kernel_wins": bool(k_s < t_s - spread),
            "chain_moves_per_s_kernel": chains * MOVES / k_s, "kernel_best_cost": float(res["k"].best_cost),
            "torch_best_cost": float(res["t"].best_cost)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sa_domains_bench.jsonl"))
    ap.add_argument("--sweep-out", default=os.path.join(ROOT, "profiles", "sa_subset_cap_sweep.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--meeting-chains", type=int, nargs="*", default=[1, 64, 4096])
    ap.add_argument("--rows", type=int, nargs="*", default=[4000, 65536])
    ap.add_argument("--subset-chains", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--sweep", action="store_true", help="also run the one-chain row sweep")
    ap.add_argument("--sweep-repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sa_domains needs a GPU")
    from avenir_amd.optimize.domains import MeetingScheduleDomain
    dev = torch.device("cuda")

    def emit(path, row):
        print(json.dumps(row), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as fh:
            fh.write(json.dumps(row) + "\n")

    d = MeetingScheduleDomain.random_instance(10, 20, seed=3, device=dev)
    for chains in args.meeting_chains:
        emit(args.out, {"bench": "sa_domains", "domain": "meeting", "meetings": 10, "people": 20,
                        **_sa_pair(d, "sa_meeting_kernel", chains, 0.5, args.repeats)})
    for n in args.rows:
        d = _subset_domain(n, dev)
        for chains in args.subset_chains:
            emit(args.out, {"bench": "sa_domains", "domain": "subset", "rows": n, "features": d.F,
                            "classes": int(d.loglik.shape[2]),
                            **_sa_pair(d, "sa_subset_kernel", chains, 0.05, args.repeats)})
    if args.sweep:
        for e in range(12, 21):
            d = _subset_domain(1 << e, dev)
            emit(args.sweep_out, {"bench": "sa_subset_cap_sweep", "domain": "subset", "rows": 1 << e, "features": d.F,
                                  "classes": int(d.loglik.shape[2]),
                                  **_sa_pair(d, "sa_subset_kernel", 1, 0.05, args.sweep_repeats)})


if __name__ == "__main__":
    main()
