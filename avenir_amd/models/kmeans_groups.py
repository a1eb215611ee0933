"""Many independent k-means fits in one launch: the device Lloyd loops of ``kmeans_groups.hip``
and their host twin.

``KMeans.fit`` streams one big table through the K16 kernels, three launches and one host read
per iteration.  The kMeansPlusPlusCluster job has the opposite shape (one model per key group,
every k, several restarts: S/cluster/KMeansPlusPlusCluster.scala): many small fits whose whole cost
is launches and round trips.  Here every (group, k, restart) run is one workgroup that iterates
from its initial centroids to convergence on the device; :func:`kmeans_groups_twin` is the same
arithmetic in numpy, bit for bit:

* distance: ``acc = 0``, then for d in order ``t = x_d - c_jd; acc = acc + t * t`` in float32,
  product and sum rounded separately; the argmin takes the lowest index on ties.  Direct
  differences need no centring, so this path does not translate the data;
* sums: exact, in 64-bit fixed point per group: ``max|x| < 2^e`` as ``frexp`` gives it (``e = 0``
  for an all-zero group), ``scale = 2^(40 - e)``, ``q = int64(rint(float64(x) * scale))``;
* update: ``new = float32(float64(S) / (float64(cnt) * scale))``, an empty cluster keeps its
  centroid;
* shift: ``sh_c = sum_d (new - old)^2`` in float32, in d order;
* convergence: ``"shift"``: ``float64(max_c sh_c) <= tol * tol``; ``"sklearn"``:
  ``float64(sum_c sh_c) <= tol_eff`` summed in c order (no square root);
* SSE: the float64 sum of the float32 best distances (the kernel adds them in a fixed order; the
  twin's order is numpy's — they agree to the reordering bound n 2^-52).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .. import _native

MAX_K = 64
MAX_D = 64
MAX_ROWS = 1 << 22


@dataclass
class GroupRun:
    """Result of one run: ``centroids`` [k, D] float32 (on the data's device), ``counts`` [k] int64
    (host), final ``sse``, ``iterations``, ``converged`` and the per-iteration SSE ``history``."""
    centroids: torch.Tensor
    counts: torch.Tensor
    sse: float
    iterations: int
    converged: bool
    history: list


def padded_dim(D: int) -> int | None:
    return next((p for p in (2, 4, 8, 16, 32, 64) if p >= D), None)


def _threshold(tol: float, tol_mode: str, tol_eff: float | None) -> float:
    if tol_mode == "shift":
        return float(tol) * float(tol)
    if tol_mode != "sklearn":
        raise ValueError(f"unknown tol_mode {tol_mode}")
    return float(tol if tol_eff is None else tol_eff)


def kmeans_groups_twin(X, C0, max_iter: int, tol: float, tol_mode: str = "shift", tol_eff: float | None = None):
    """One run of the device loop in numpy -> (centroids f32 [k, D], counts i64 [k], sse, iterations,
    converged, history).  ``X`` [n, D] and ``C0`` [k, D] are float32 (unpadded: zero padding adds
    exact zeros).  Raises ``ValueError`` on non-finite data."""
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float32))
    C = np.array(np.asarray(C0, dtype=np.float32), copy=True)
    n, D = X.shape
    k = C.shape[0]
    thr = _threshold(tol, tol_mode, tol_eff)
    mx = np.float32(np.abs(X).max()) if X.size else np.float32(0)
    if not np.isfinite(mx):
        raise ValueError("k-means: the data holds a non-finite value")
    e = 0 if mx == 0 else int(np.frexp(np.float64(mx))[1])
    scale = np.ldexp(np.float64(1.0), 40 - e)
    Q = np.rint(X.astype(np.float64) * scale).astype(np.int64)
    ar = np.arange(n)

    def assign(C):
        acc = np.zeros((k, n), dtype=np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            for d in range(D):
                t = X[None, :, d] - C[:, None, d]
                acc = acc + t * t
        idx = acc.argmin(0)                      # first minimum: the lowest index on ties
        best = acc[idx, ar]
        return idx, np.bincount(idx, minlength=k).astype(np.int64), float(best.astype(np.float64).sum())

    history, it, done = [], 0, False
    while it < max_iter and not done:
        idx, cnt, sse = assign(C)
        history.append(sse)
        S = np.zeros((k, D), dtype=np.int64)
        np.add.at(S, idx, Q)
        den = np.maximum(cnt, 1).astype(np.float64) * scale
        new = np.where(cnt[:, None] > 0, (S.astype(np.float64) / den[:, None]).astype(np.float32), C)
        sh = np.zeros(k, dtype=np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            for d in range(D):
                t = new[:, d] - C[:, d]
                sh = sh + t * t
        if tol_mode == "shift":
            agg = sh.max()
        else:
            agg = sh[0]
            for c in range(1, k):
                agg = np.float32(agg + sh[c])
        done = bool(np.float64(agg) <= thr)
        C = new.astype(np.float32)
        it += 1
    _, cnt, sse = assign(C)
    return C, cnt, sse, it, done, history


def kmeans_fit_groups(Xs: list[torch.Tensor], run_group: list[int], inits: list[torch.Tensor], max_iter: int,
                      tol: float, tol_mode: str = "shift", tol_effs: list[float] | None = None,
                      device: torch.device | str | None = None) -> list[GroupRun]:
    """Fit run r (initial centroids ``inits[r]`` [k_r, D]) on group ``Xs[run_group[r]]`` [n_g, D], all
    runs of the call at once.  ``tol_effs[r]`` is run r's threshold in ``"sklearn"`` mode.  On a
    CUDA ``device`` the runs share one ``kmeans_fit_groups`` call of the extension (one workgroup
    per run; the outputs come back with one read per array); on the CPU each run goes through
    :func:`kmeans_groups_twin`.  Non-finite data raises ``ValueError``."""
    if not Xs or not inits:
        return []
    device = torch.device(device) if device is not None else Xs[0].device
    D = Xs[0].shape[1]
    if any(X.dim() != 2 or X.shape[1] != D for X in Xs) or any(C.dim() != 2 or C.shape[1] != D for C in inits):
        raise ValueError("k-means groups: every group and every init must be [*, D] with one D")
    if len(run_group) != len(inits) or any(g < 0 or g >= len(Xs) for g in run_group):
        raise ValueError("k-means groups: a run points past the group table")
    R = len(inits)
    thr = [_threshold(tol, tol_mode, None if tol_effs is None else tol_effs[r]) for r in range(R)]
    if device.type != "cuda":
        out = []
        for r in range(R):
            C, cnt, sse, it, done, hist = kmeans_groups_twin(
                Xs[run_group[r]].detach().cpu().numpy(), inits[r].detach().cpu().numpy(), max_iter, tol, tol_mode,
                None if tol_effs is None else tol_effs[r])
            out.append(GroupRun(torch.from_numpy(C), torch.from_numpy(cnt), sse, it, done, hist))
        return out
    Dp = padded_dim(D)
    if Dp is None:
        raise ValueError(f"k-means groups: D={D} exceeds {MAX_D}")
    ks = [int(C.shape[0]) for C in inits]
    ns = [int(X.shape[0]) for X in Xs]
    if len(Xs) == 1 and Dp == D:
        Xp = Xs[0].to(device=device, dtype=torch.float32).contiguous()
    else:
        Xp = torch.zeros((sum(ns), Dp), dtype=torch.float32, device=device)
        Xp[:, :D] = torch.cat([X.to(device) for X in Xs])
    C0 = torch.zeros((sum(ks), Dp), dtype=torch.float32, device=device)
    C0[:, :D] = torch.cat([C.to(device) for C in inits])
    goff = np.concatenate([[0], np.cumsum(ns)[:-1]]).astype(np.int64)
    coff = np.concatenate([[0], np.cumsum(ks)[:-1]]).astype(np.int64)
    groups = torch.from_numpy(np.stack([goff, np.asarray(ns, dtype=np.int64)], 1))
    runs = torch.from_numpy(np.stack([np.asarray(run_group, dtype=np.int64), np.asarray(ks, dtype=np.int64), coff], 1))
    res = _native.C().kmeans_fit_groups(Xp, groups, runs, C0, torch.tensor(thr, dtype=torch.float64), D,
                                        int(max_iter), 0 if tol_mode == "shift" else 1)
    Cd = res[0] if Dp == D else res[0][:, :D].contiguous()
    counts, sse, iters, conv, hist, status = (t.cpu() for t in res[1:])     # one read per array
    if bool(status.any()):
        raise ValueError("k-means: the data holds a non-finite value")
    counts = counts.long()
    sse, iters, conv, hist = sse.tolist(), iters.tolist(), conv.tolist(), hist.tolist()
    Cv, nv = Cd.split(ks), counts.split(ks)        # every run's view in one call each
    return [GroupRun(Cv[r], nv[r], sse[r], iters[r], bool(conv[r]), hist[r][:iters[r]]) for r in range(R)]
