"""DBSCAN with a fixed fp32 neighbour predicate: the numpy twin that defines the arithmetic, and
the model that runs it on the device kernels (csrc/kernels/dbscan.hip).

Reference: ``train.algo=dbscan`` of P/unsupv/cluster.py (sklearn's DBSCAN).  With the predicate
fixed, the whole output depends on no execution order:

* ``s(i, j)`` is the fp32 sum over the columns of ``t * t`` (euclidean) or ``|t|`` (manhattan) with
  ``t = x[i, d] - x[j, d]``; the subtraction, the square and every add are rounded on their own.
  The even columns are summed in one chain in ascending ``d``, the odd columns in another, and
  ``s = even + odd`` (the two halves of a packed fp32 register on the device).  Zero padding
  columns add exact zeros, and ``s`` is symmetric in ``(i, j)``.
* ``j`` is a neighbour of ``i`` iff ``s <= thr``: for the euclidean metric ``thr =
  eps_sq_threshold(eps)``, the largest finite fp32 ``v`` with ``sqrt_f32(v) <= float32(eps)`` (the
  predicate ``sqrtf(s) <= eps`` of a correctly rounded square root, with no square root in the
  sweep); for manhattan ``thr = float32(eps)``.
* ``counts[i]`` counts the neighbours of ``i``, itself included; ``i`` is core iff ``counts[i] >=
  min_samples``.  A cluster is a connected component of the core graph, its root the smallest point
  index in it; a non-core point takes the smallest root among its core neighbours, or -1 (noise).
  Roots are renumbered 0..m-1 in ascending order: the order in which sklearn's index scan opens the
  clusters, and the cluster sklearn's expansion reaches a shared border point from first.
"""
from __future__ import annotations

import numpy as np
import torch

METRICS = {"euclidean": 0, "manhattan": 1}
_F32_MAX = np.finfo(np.float32).max


def eps_sq_threshold(eps: float) -> np.float32:
    """The largest finite fp32 ``v`` with ``sqrt_f32(v) <= float32(eps)``."""
    e = np.float32(eps)
    if not (e >= 0):
        raise ValueError("eps must be >= 0")
    if not np.isfinite(e):
        return _F32_MAX
    with np.errstate(over="ignore"):
        v = np.float32(e * e)
    if not np.isfinite(v):
        v = _F32_MAX
    ninf, pinf = np.float32(-np.inf), np.float32(np.inf)
    while np.sqrt(v) > e:
        v = np.nextafter(v, ninf)
    while v < _F32_MAX and np.sqrt(np.nextafter(v, pinf)) <= e:
        v = np.nextafter(v, pinf)
    return np.float32(v)


def _threshold(eps: float, metric: str) -> np.float32:
    return eps_sq_threshold(eps) if metric == "euclidean" else np.float32(eps)


def _check_params(eps, min_samples, metric):
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}")
    if not (np.isfinite(eps) and eps >= 0):
        raise ValueError("eps must be finite and >= 0")
    if int(min_samples) != min_samples or min_samples < 1:
        raise ValueError("min_samples must be an integer >= 1")


def _check_shape(shape, dtype_ok):
    if not dtype_ok:
        raise ValueError("X must be float32")
    if len(shape) != 2 or shape[0] < 1 or not 1 <= shape[1] <= 64:
        raise ValueError("X must be [n, D] with n >= 1 and 1 <= D <= 64")


def _pair_sums(A: np.ndarray, Bt: np.ndarray, metric: str) -> np.ndarray:
    """s [len(A), nB] for the rows of A against the columns of Bt [D, nB], in the contract's order;
    every numpy operation rounds to fp32."""
    acc = [np.zeros((A.shape[0], Bt.shape[1]), dtype=np.float32) for _ in range(2)]
    t = np.empty_like(acc[0])
    for d in range(A.shape[1]):
        np.subtract(A[:, d, None], Bt[d][None, :], out=t)
        if metric == "euclidean":
            np.multiply(t, t, out=t)
        else:
            np.abs(t, out=t)
        acc[d & 1] += t
    return np.add(acc[0], acc[1], out=t)


def _find(parent: np.ndarray, x: np.ndarray) -> np.ndarray:
    while True:
        p = parent[x]
        if np.array_equal(p, x):
            return x
        x = p


def dbscan_twin(X, eps: float, min_samples: int, metric: str = "euclidean", chunk: int = 256):
    """(labels int64 [n], counts int32 [n]) by the definition above, in row chunks of ``chunk`` so
    that memory stays O(chunk * n)."""
    _check_params(eps, min_samples, metric)
    X = np.asarray(X)
    _check_shape(X.shape, X.dtype == np.float32)
    if not np.isfinite(X).all():
        raise ValueError("X must be finite")
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    n = X.shape[0]
    thr = _threshold(eps, metric)
    counts = np.zeros(n, dtype=np.int32)
    Xt = np.ascontiguousarray(X.T)
    for s in range(0, n, chunk):
        counts[s:s + chunk] = (_pair_sums(X[s:s + chunk], Xt, metric) <= thr).sum(1)
    core = counts >= min_samples
    cidx = np.flatnonzero(core)
    Xc, Xct = X[cidx], np.ascontiguousarray(Xt[:, cidx])
    nc = len(cidx)
    # components of the core graph: every row hooks the roots of its neighbours under the smallest
    parent = np.arange(nc, dtype=np.int64)
    for s in range(0, nc, chunk):
        adj = _pair_sums(Xc[s:s + chunk], Xct, metric) <= thr
        for r in range(adj.shape[0]):
            nb = np.flatnonzero(adj[r])                       # the row itself is among them
            roots = _find(parent, nb)
            parent[roots] = parent[nb] = roots.min()
    root = _find(parent, np.arange(nc, dtype=np.int64))
    # border points: the smallest root among the core neighbours
    min_root = np.full(n, nc, dtype=np.int64)
    min_root[cidx] = root
    bidx = np.flatnonzero(~core & (counts >= 2))
    for s in range(0, len(bidx), chunk):
        if nc == 0:
            break
        adj = _pair_sums(X[bidx[s:s + chunk]], Xct, metric) <= thr
        min_root[bidx[s:s + chunk]] = np.where(adj, root[None, :], nc).min(1)
    return _renumber_np(min_root, root, nc), counts


def _renumber_np(min_root, root, nc):
    ids = np.cumsum(root == np.arange(nc)) - 1          # root -> cluster id, ascending in the root
    ids = np.append(ids, -1).astype(np.int64)           # nc = no core neighbour
    return ids[min_root]


class DBSCAN:
    """``fit(X)`` / ``fit_predict(X)`` with sklearn's attribute names.  A CUDA tensor runs the device
    kernels, a CPU tensor (or numpy array) the twin; ``use_kernel=False`` runs the twin on a host
    copy of a CUDA tensor, ``use_kernel=True`` insists on the kernels.  Both give the same bits."""

    def __init__(self, eps: float = 0.5, min_samples: int = 5, metric: str = "euclidean", use_kernel=None,
                 a_range: int = 0):
        _check_params(eps, min_samples, metric)
        self.eps, self.min_samples, self.metric = float(eps), int(min_samples), metric
        self.use_kernel, self.a_range = use_kernel, int(a_range)

    def fit(self, X) -> "DBSCAN":
        if not isinstance(X, torch.Tensor):
            X = torch.from_numpy(np.ascontiguousarray(X))
        _check_shape(tuple(X.shape), X.dtype == torch.float32)
        kernel = X.is_cuda if self.use_kernel is None else bool(self.use_kernel)
        if kernel and not X.is_cuda:
            raise ValueError("use_kernel=True needs a CUDA tensor")
        if kernel:
            labels, counts = self._fit_device(X.contiguous())
        else:
            lab, cnt = dbscan_twin(X.detach().cpu().numpy(), self.eps, self.min_samples, self.metric)
            labels, counts = torch.from_numpy(lab).to(X.device), torch.from_numpy(cnt).to(X.device)
        self.labels_, self.counts_ = labels, counts
        self.core_sample_indices_ = (counts >= self.min_samples).nonzero().view(-1)
        self.n_clusters_ = int(labels.max()) + 1
        return self

    def fit_predict(self, X) -> torch.Tensor:
        return self.fit(X).labels_

    def _fit_device(self, X: torch.Tensor):
        from .. import _native
        C = _native.C()
        if not bool(torch.isfinite(X).all()):
            raise ValueError("X must be finite")
        met, thr, rg = METRICS[self.metric], float(_threshold(self.eps, self.metric)), self.a_range
        n = X.shape[0]
        counts = C.dbscan_count(X, met, thr, rg)
        core = counts >= self.min_samples
        cidx = core.nonzero().view(-1)                  # ascending original index
        nc = cidx.numel()
        min_root = torch.full((n,), nc, dtype=torch.int64, device=X.device)
        ids = torch.full((nc + 1,), -1, dtype=torch.int64, device=X.device)
        if nc:
            Xc = X[cidx].contiguous()
            root = C.dbscan_union(Xc, met, thr, rg)     # int32, flattened
            min_root[cidx] = root.long()
            bidx = (~core & (counts >= 2)).nonzero().view(-1)   # only these can be border points
            if bidx.numel():
                mr = C.dbscan_border(X[bidx].contiguous(), Xc, root, met, thr, rg).long()
                min_root[bidx] = mr.clamp_max(nc)       # INT_MAX: no core neighbour
            ids[:nc] = torch.cumsum(root == torch.arange(nc, device=X.device), 0) - 1
        return ids[min_root], counts
