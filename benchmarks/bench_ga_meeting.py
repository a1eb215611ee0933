#!/usr/bin/env python3
"""Island GA over the meeting-schedule domain on one GPU: the one-launch island kernel
(optimize/ga_meeting.py, csrc/kernels/optim.hip::ga_meeting_kernel) against the per-island torch
path (GeneticAlgorithm(use_kernel=False): about a dozen small launches per island and generation).

The reference configuration (resource/mesched.properties): 10 meetings, 20 people, pool 30,
mating 10, replacement 10, children join the pool, 100 generations.  Kernel path at 1, 64, 256 and
4096 islands, torch path at 1 and 64 islands only (its launch count makes larger sizes pointless).

Two times per kernel configuration, each the median of ``--repeats`` synchronised runs after a
warm-up: ``run_s`` is a whole ``GeneticAlgorithm.run()`` (host-side initial pools, upload, launch,
download — what the torch path's ``run_s`` also covers), ``kernel_s`` is one call of the binding with
the pools resident on the device (its argument checks, a device copy of the pools, the launch).  One
JSON line each, printed and written to ``--out``."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

M, Q, P, MATING, R, G = 10, 20, 30, 10, 10, 100


def _median_s(fn, repeats: int) -> tuple[float, list[float]]:
    fn()                                                   # warm-up
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "ga_meeting_bench.jsonl"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-repeats", type=int, default=5)
    ap.add_argument("--islands", type=int, nargs="*", default=[1, 64, 256, 4096])
    ap.add_argument("--torch-islands", type=int, nargs="*", default=[1, 64])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ga_meeting needs a GPU")
    from avenir_amd import _native
    from avenir_amd.optimize.domains import MeetingScheduleDomain
    from avenir_amd.optimize.ga_meeting import (_device_tables, ga_meeting_init, ga_meeting_lds, ga_meeting_price,
                                                meeting_tables)
    from avenir_amd.optimize.search import GeneticAlgorithm
    dev = torch.device("cuda")
    d = MeetingScheduleDomain.random_instance(M, Q, seed=3, device=dev)
    tb = meeting_tables(d)
    rows = []

    def emit(row):
        row = {"bench": "ga_meeting", "meetings": M, "people": Q, "pool": P, "mating": MATING, "replacement": R,
               "purge_first": False, "generations": G, **row}
        rows.append(row)
        print(json.dumps(row), flush=True)

    kw = dict(pool=P, mating=MATING, replacement=R, generations=G, purge_first=False, seed=1)
    for islands in args.islands:
        ga = GeneticAlgorithm(d, islands=islands, use_kernel=True, **kw)
        res = []
        run_s, runs = _median_s(lambda: res.append(ga.run()), args.repeats)
        assert res[-1].stats["engine"] == "ga_meeting_kernel"
        pop = ga_meeting_init(tb, islands, P, 1, 0)
        tp0 = torch.from_numpy(pop).to(dev)
        tc0 = torch.from_numpy(ga_meeting_price(tb, pop)).to(dev)
        hist = torch.empty((islands, G), dtype=torch.float32, device=dev)
        dom = _device_tables(tb, dev)

        def launch():
            tp, tc = tp0.clone(), tc0.clone()
            _native.C().ga_meeting(*dom, float("inf"), tp, tc, hist, G, MATING, R, False, True, 1, 0, 0)

        kernel_s, launches = _median_s(launch, args.repeats)
        emit({"impl": "island_kernel", "islands": islands, "run_s": run_s, "run_s_all": runs, "kernel_s": kernel_s,
              "kernel_s_all": launches, "island_generations_per_s": islands * G / run_s,
              "kernel_island_generations_per_s": islands * G / kernel_s, "lds_bytes": ga_meeting_lds(P, 3 * M, R),
              "best_cost": float(res[-1].best_cost)})
    for islands in args.torch_islands:
        ga = GeneticAlgorithm(d, islands=islands, use_kernel=False, **kw)
        res = []
        run_s, runs = _median_s(lambda: res.append(ga.run()), args.torch_repeats)
        assert "engine" not in res[-1].stats
        emit({"impl": "per_island_torch", "islands": islands, "run_s": run_s, "run_s_all": runs,
              "island_generations_per_s": islands * G / run_s, "best_cost": float(res[-1].best_cost)})
    by = {(r["impl"], r["islands"]): r for r in rows}
    for islands in args.torch_islands:
        k, t = by.get(("island_kernel", islands)), by.get(("per_island_torch", islands))
        if k and t:
            emit({"impl": "ratio", "islands": islands, "torch_run_s_over_kernel_run_s": t["run_s"] / k["run_s"]})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for row in rows:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
