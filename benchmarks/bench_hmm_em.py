#!/usr/bin/env python3
"""Baum-Welch training on one GPU: the one-launch E-step kernel (models/hmm_em.py,
csrc/kernels/hmm.hip::hmm_estep_kernel) and a whole 10-iteration ``fit_unsupervised``.

Shapes (sequences x steps x states x symbols): 2^20 x 64 x 8 x 16, the README's Viterbi shape, and
2^14 x 256 x 32 x 16; uniform random observations from a seed, every row full length.

* ``estep``: one ``hmm_estep`` call (zeroed tables, every chunk's launch, no host read) against
  (a) ``torch_estep`` below, a batched scaled forward-backward in fp32 torch ops on the same GPU
  (2 T small launches of matmuls, gathers and an index_add per step), timed in alternating pairs;
  and (b) ``viterbi(..., forward=True)``, the forward log-likelihood kernel, at the same shape: the
  E-step is a forward pass, a backward pass and S^2 pair posteriors per step, so its time is also
  reported as a multiple of the forward pass.  The tables of kernel and torch path are compared
  once (largest relative difference of a cell): against the timed fp32 path, whose sums over the
  batch are fp32 atomics in an undefined order and lose digits as the batch grows, and against the
  same path with fp64 sums.
* ``caps``: the E-step at several workspace caps (the number of launches the rows are split into).
* ``fit``: 10 iterations of ``fit_unsupervised`` from a seeded start, once with ``tol=None`` (no
  per-sequence read-back) and once testing the log-likelihood every iteration without ever
  stopping; the difference is the share of an iteration spent on the Z / E read-back and the host
  log.

Every time is a host clock around work that ends in a device synchronise, after one warm-up of
each shape; medians of ``--repeats`` alternating runs with the min-max spread.  The kernel alone
under a profiler and multi-GPU runs are not measured here.  One JSON line per measurement, printed
and appended to ``--out``."""
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

SHAPES = [(1 << 20, 64, 8, 16), (1 << 14, 256, 32, 16)]
FIT_ITERS = 10


def torch_estep(obs, A, B, pi, acc=torch.float32):
    """Scaled forward-backward over the batch in fp32 torch ops: (trans, emit, init, log-likelihood).
    ``acc`` is the dtype of the three sums over the batch (fp64 for the accuracy check)."""
    N, T = obs.shape
    S, O = B.shape
    o = obs.long()
    Bt = B.t().contiguous()
    alpha = torch.empty((T, N, S), dtype=torch.float32, device=obs.device)
    c = torch.empty((T, N), dtype=torch.float32, device=obs.device)
    for t in range(T):
        a = (pi if t == 0 else alpha[t - 1] @ A) * Bt[o[:, t]]
        c[t] = a.sum(1)
        alpha[t] = a / c[t][:, None]
    beta = torch.ones((N, S), dtype=torch.float32, device=obs.device)
    trans = torch.zeros((S, S), dtype=acc, device=obs.device)
    emit = torch.zeros((O, S), dtype=acc, device=obs.device)
    init = None
    for t in range(T - 1, -1, -1):
        g = (alpha[t] * beta).to(acc)
        emit.index_add_(0, o[:, t], g)
        if t == 0:
            init = g.sum(0)
        else:
            w = Bt[o[:, t]] * beta / c[t][:, None]
            trans += alpha[t - 1].t().to(acc) @ w.to(acc)
            beta = w @ A.t()
    return trans * A, emit.t(), init, c.double().log().sum()


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _alternating(fns: dict, repeats: int) -> dict:
    for f in fns.values():      # one warm-up each
        f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            ts[k].append(_timed(f))
    return {k: {"median_ms": 1e3 * statistics.median(v), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v)}
            for k, v in ts.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hmm_em_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hmm_em needs a GPU")
    from avenir_amd.models import hmm_em as H
    from avenir_amd.models.markov import HiddenMarkovModelBuilder
    from avenir_amd.ops import sequence_ops as SO
    dev = torch.device("cuda:0")

    def emit(rec):
        rec = {"bench": "hmm_em", "device": torch.cuda.get_device_name(0), **rec}
        line = json.dumps(rec)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    for N, T, S, O in SHAPES:
        shape = {"sequences": N, "steps": T, "states": S, "symbols": O}
        g = torch.Generator().manual_seed(N + T)
        obs = torch.randint(0, O, (N, T), generator=g, dtype=torch.int16).to(dev)
        A, B, pi = (torch.from_numpy(x).float().to(dev) for x in H.random_start(S, O, 1))
        lA, lB, lp = A.log(), B.log(), pi.log()
        per_row = T * (S + 1) * 4
        cap = H.DEFAULT_WORKSPACE_BYTES
        launches = -(-N // max(1, min(N, cap // per_row)))
        r = _alternating({"kernel": lambda: H.hmm_estep(obs, A, B, pi),
                          "forward": lambda: SO.viterbi(obs, lA, lB, lp, forward=True),
                          "torch": lambda: torch_estep(obs, A, B, pi)}, args.repeats)
        rec = {"what": "estep", **shape, "workspace_cap_bytes": cap, "launches": launches, **
               {f"{k}_{m}": round(v[m], 4) for k, v in r.items() for m in v}}
        k = r["kernel"]["median_ms"]
        rec["kernel_steps_per_s"] = round(N * T / (k * 1e-3), 1)
        rec["kernel_over_forward"] = round(k / r["forward"]["median_ms"], 3)
        rec["torch_over_kernel"] = round(r["torch"]["median_ms"] / k, 3)
        spread = max(r["kernel"]["max_ms"] - r["kernel"]["min_ms"], r["torch"]["max_ms"] - r["torch"]["min_ms"])
        rec["kernel_wins"] = bool(r["torch"]["median_ms"] - k > spread)
        tq, eq, iq, Z, E, _ = H.hmm_estep(obs, A, B, pi)
        f = lambda q: q.double() * 2.0 ** -H.COUNT_FRAC_BITS
        for name, acc in (("fp32_sums", torch.float32), ("fp64_sums", torch.float64)):
            tt, te, ti, tll = torch_estep(obs, A, B, pi, acc)
            rec[f"max_rel_diff_vs_torch_{name}"] = max(
                float(((f(q) - x.double()).abs() / x.double().clamp_min(1e-3)).max())
                for q, x in ((tq, tt), (eq, te), (iq, ti)))
            del tt, te, ti
        rec["loglik_kernel"] = H.loglik_fixed(Z, E) * 2.0 ** -H.LL_FRAC_BITS
        rec["loglik_torch"] = float(tll)
        emit(rec)

        caps = {f"{c >> 20}MiB": c for c in (32 << 20, 128 << 20, 512 << 20, 1024 << 20, 4096 << 20)}
        rc = _alternating({n: (lambda c=c: H.hmm_estep(obs, A, B, pi, workspace_bytes=c)) for n, c in caps.items()},
                          args.repeats)
        emit({"what": "caps", **shape, **{f"{n}_launches": -(-N // max(1, min(N, c // per_row))) for n, c in caps.items()},
              **{f"{n}_{m}": round(v[m], 4) for n, v in rc.items() for m in v}})

        b = HiddenMarkovModelBuilder([f"s{i}" for i in range(S)], [f"o{i}" for i in range(O)])
        rf = _alternating({"blind": lambda: b.fit_unsupervised(obs, iters=FIT_ITERS, tol=None, seed=2),
                           # a negative tolerance never stops: the log-likelihood is tested every iteration
                           "tested": lambda: b.fit_unsupervised(obs, iters=FIT_ITERS, tol=-1.0, seed=2)}, args.repeats)
        fit = b.fit_unsupervised(obs, iters=FIT_ITERS, tol=-1.0, seed=2)
        assert fit.iterations == FIT_ITERS and len(fit.log_likelihood) == FIT_ITERS
        emit({"what": "fit", **shape, "iterations": FIT_ITERS, "workspace_cap_bytes": cap,
              **{f"{k}_{m}": round(v[m], 4) for k, v in rf.items() for m in v},
              "readback_and_log_share": round(1 - rf["blind"]["median_ms"] / rf["tested"]["median_ms"], 4),
              "log_likelihood_first": fit.log_likelihood[0], "log_likelihood_last": fit.log_likelihood[-1]})
        del obs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
