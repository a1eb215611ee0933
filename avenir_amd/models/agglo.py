"""Agglomerative clustering by rounds of reciprocal nearest pairs: the numpy twin that defines the
arithmetic, and the model that runs it on the device kernels (csrc/kernels/agglo.hip).

Reference: ``train.algo=agglomerative`` of P/unsupv/cluster.py (sklearn's AgglomerativeClustering).
For the reducible linkages (single, complete, average, ward) every pair of mutually nearest clusters
can be merged in the same round without changing the dendrogram, so a fit is a few dozen sweeps over
a dense fp32 matrix rather than ``n - 1`` dependent steps.  The contract, which fixes every bit:

* ``M`` is ``n x n`` fp32 with ``+inf`` on the diagonal.  ``s(i, j)`` is the pair sum of
  :func:`avenir_amd.models.dbscan._pair_sums`.  Euclidean with single, complete or average linkage
  stores ``sqrt_f32(s)`` (correctly rounded), manhattan stores ``s``; ward stores the squared
  euclidean ``s`` and reports ``sqrt_f32`` of the stored height.  An off-diagonal entry above
  ``2**96`` is refused, so that a cluster size times an entry stays finite.
* A round: ``nn[k]`` is the column of the smallest entry of row ``k`` (ties: the smallest column);
  every ``i < j`` with ``nn[i] = j`` and ``nn[j] = i`` merges, slot ``i`` survives and slot ``j``
  dies.  The pair holding the globally smallest key is always reciprocal, so a fit takes at most
  ``n - 1`` rounds.
* New distances are Lance-Williams in fp32, every operation rounded on its own (``a = d(i, k)``,
  ``b = d(j, k)``, ``c = d(i, j)``, sizes exact in fp32): single ``min(a, b)``, complete
  ``max(a, b)``, average ``max((n_i * a + n_j * b) / (n_i + n_j), c)``, ward ``max((((n_i + n_k) * a
  + (n_j + n_k) * b) - n_k * c) / ((n_i + n_j) + n_k), c)``.  The clamp at ``c`` keeps the heights
  along any root path from decreasing.
* The pairs of one round are applied as if one after the other in ascending order of the surviving
  slot.  The matrix stays symmetric bit for bit, so everything the new row of a survivor needs lies
  in its own old row and in the row of its dead partner, and a row that does not merge needs only
  itself: no update reads what another one writes.
* The merges ``(stored height, round, i, j)`` are sorted by ``(height bits, round, i)``; children
  precede parents under this key.  ``children_`` / ``distances_`` follow sklearn's layout: merge
  ``t`` creates node ``n + t``, the smaller id first.
* Labels: the first ``n - n_clusters`` merges are applied, or with ``distance_threshold`` every merge
  whose reported height is ``< float32(threshold)``; clusters are numbered by their smallest member
  index, ascending (DBSCAN's convention).

Not covered: a matrix-free path for large ``n`` (the matrix is dense, ``max_matrix_bytes`` bounds
it), a Boruvka spanning-tree path for single linkage, cosine and precomputed affinities, and
connectivity constraints.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from .dbscan import METRICS, _check_shape, _pair_sums

LINKAGES = {"single": 0, "complete": 1, "average": 2, "ward": 3}
ENTRY_LIMIT = np.float32(2.0 ** 96)
# Default dispatch (use_kernel=None): a CUDA tensor of fewer rows runs the twin on a host copy.  A fit
# costs a handful of launches and one counter read per round whatever its size; whole fits at n = 32
# took 0.65 ms on the kernels against 0.42-0.50 ms on the twin, at n = 128 0.9-1.1 ms against
# 1.2-1.6 ms, and from n = 1024 on the kernels were 7 to 97 times faster (profiles/agglo_bench.jsonl).
# Sizes between 32 and 128 were not measured.
KERNEL_MIN_ROWS = 128
_INF = np.float32(np.inf)


class AggloResult(NamedTuple):
    children: np.ndarray        # int64 [n - 1, 2]
    distances: np.ndarray       # float32 [n - 1]
    labels: np.ndarray          # int64 [n]
    rounds: int


def _check_params(linkage, metric, n_clusters, distance_threshold):
    if linkage not in LINKAGES:
        raise ValueError(f"linkage must be one of {sorted(LINKAGES)}")
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}")
    if linkage == "ward" and metric != "euclidean":
        raise ValueError("ward linkage takes the euclidean metric only")
    if (n_clusters is None) == (distance_threshold is None):
        raise ValueError("exactly one of n_clusters and distance_threshold must be given")
    if n_clusters is not None and (int(n_clusters) != n_clusters or n_clusters < 1):
        raise ValueError("n_clusters must be an integer >= 1")
    if distance_threshold is not None and np.isnan(distance_threshold):
        raise ValueError("distance_threshold must not be NaN")


def _check_cut(n, n_clusters):
    if n_clusters is not None and not 1 <= n_clusters <= n:
        raise ValueError(f"n_clusters must lie in 1 .. n = {n}")


def _takes_sqrt(linkage, metric):
    return metric == "euclidean" and linkage != "ward"


def leading_dim(n: int) -> int:
    """Floats per matrix row on the device: whole 16-byte groups."""
    return (n + 3) // 4 * 4


def _check_bytes(n, max_matrix_bytes):
    need = n * leading_dim(n) * 4
    if need > max_matrix_bytes:
        raise ValueError(f"the {n} x {n} fp32 matrix takes {need} bytes, above max_matrix_bytes = {max_matrix_bytes}")


def _initial_matrix(X: np.ndarray, linkage: str, metric: str, chunk: int = 256) -> np.ndarray:
    n = X.shape[0]
    M = np.empty((n, n), dtype=np.float32)
    Xt = np.ascontiguousarray(X.T)
    with np.errstate(over="ignore"):                                  # an overflow is refused below
        for s in range(0, n, chunk):
            M[s:s + chunk] = _pair_sums(X[s:s + chunk], Xt, metric)
    if _takes_sqrt(linkage, metric):
        np.sqrt(M, out=M)
    np.fill_diagonal(M, 0)
    if n and not M.max() <= ENTRY_LIMIT:
        raise ValueError("a distance matrix entry exceeds 2**96")
    np.fill_diagonal(M, _INF)
    return M


def _lance_williams(linkage, a, b, c, ni, nj, nk):
    """fp32 throughout: ``ni``, ``nj``, ``c`` are np.float32 scalars, ``a``, ``b``, ``nk`` fp32 arrays."""
    if linkage == "single":
        return np.minimum(a, b)
    if linkage == "complete":
        return np.maximum(a, b)
    if linkage == "average":
        return np.maximum((ni * a + nj * b) / (ni + nj), c)
    return np.maximum((((ni + nk) * a + (nj + nk) * b) - nk * c) / ((ni + nj) + nk), c)


def _merge_rounds(M: np.ndarray, linkage: str):
    """Runs the rounds on ``M`` (destroyed).  Returns the merge records in the order they were
    made, (height fp32, round, i, j), and the number of rounds."""
    n = M.shape[0]
    size = np.ones(n, dtype=np.int64)
    act = np.arange(n)
    h, rnd = np.empty(n - 1, dtype=np.float32), np.empty(n - 1, dtype=np.int64)
    si, sj = np.empty(n - 1, dtype=np.int64), np.empty(n - 1, dtype=np.int64)
    done = rounds = 0
    f32 = np.float32
    while len(act) > 1:
        if rounds >= n - 1:
            raise RuntimeError("agglomeration did not finish in n - 1 rounds")
        nn = np.full(n, -1, dtype=np.int64)
        nn[act] = (M if len(act) == n else M[act]).argmin(1)          # first minimum: the smallest column
        recip = act[(nn[nn[act]] == act) & (act < nn[act])]           # ascending survivors
        if not len(recip):
            raise RuntimeError("no reciprocal pair: the matrix is not symmetric")
        for i in recip:
            j = nn[i]
            c = M[i, j]
            h[done], rnd[done], si[done], sj[done] = c, rounds, i, j
            done += 1
            idx = np.flatnonzero(size > 0)
            idx = idx[(idx != i) & (idx != j)]
            new = _lance_williams(linkage, M[i, idx], M[j, idx], c, f32(size[i]), f32(size[j]), size[idx].astype(f32))
            M[i, idx] = new
            M[idx, i] = new
            M[j, :] = _INF
            M[:, j] = _INF
            size[i] += size[j]
            size[j] = 0
        act = np.flatnonzero(size > 0)
        rounds += 1
    return h, rnd, si, sj, rounds


def _dendrogram(n, h, rnd, si, sj, linkage):
    """sklearn's ``children_`` / ``distances_`` from unordered merge records, and the merged slots
    in the sorted order."""
    order = np.lexsort((si, rnd, np.ascontiguousarray(h, dtype=np.float32).view(np.int32)))
    h, si, sj = h[order], si[order].astype(np.int64), sj[order].astype(np.int64)
    node = np.arange(n, dtype=np.int64)
    children = np.empty((n - 1, 2), dtype=np.int64)
    for t in range(n - 1):
        a, b = node[si[t]], node[sj[t]]
        children[t] = (a, b) if a < b else (b, a)
        node[si[t]] = n + t
    distances = np.sqrt(h) if linkage == "ward" else h
    return children, distances.astype(np.float32), si, sj


def _cut(n, si, sj, distances, n_clusters, distance_threshold):
    if n_clusters is not None:
        m = n - int(n_clusters)
    else:
        m = int(np.searchsorted(distances, np.float32(distance_threshold), side="left"))
    root = np.arange(n, dtype=np.int64)
    root[sj[:m]] = si[:m]                                             # a dead slot hangs under a smaller one
    while True:
        nxt = root[root]
        if np.array_equal(nxt, root):
            break
        root = nxt
    ids = np.cumsum(root == np.arange(n)) - 1                         # numbered by the smallest member
    return ids[root].astype(np.int64)


def _as_input(X):
    X = np.asarray(X)
    _check_shape(X.shape, X.dtype == np.float32)
    if not np.isfinite(X).all():
        raise ValueError("X must be finite")
    return X


def agglo_twin(X, linkage: str = "ward", metric: str = "euclidean", n_clusters=None, distance_threshold=None,
               max_matrix_bytes: int = 1 << 30) -> AggloResult:
    """The whole fit by the definition above, in numpy."""
    _check_params(linkage, metric, n_clusters, distance_threshold)
    X = _as_input(X)
    n = X.shape[0]
    _check_cut(n, n_clusters)
    _check_bytes(n, max_matrix_bytes)
    M = _initial_matrix(X, linkage, metric)
    records = _merge_rounds(M, linkage)
    children, distances, si, sj = _dendrogram(n, *records[:4], linkage)
    return AggloResult(children, distances, _cut(n, si, sj, distances, n_clusters, distance_threshold), records[4])


class AgglomerativeClustering:
    """``fit(X)`` / ``fit_predict(X)`` with sklearn's attribute names (``labels_``, ``children_``,
    ``distances_``, ``n_clusters_``, ``n_leaves_``) and ``rounds_``.  A CUDA tensor runs the device
    kernels (from ``KERNEL_MIN_ROWS`` rows on; below that the twin on a host copy is faster), a CPU
    tensor (or numpy array) the twin; ``use_kernel=False`` runs the twin on a host copy of a CUDA
    tensor, ``use_kernel=True`` insists on the kernels.  Both give the same bits.

    The matrix is dense: a fit whose matrix would exceed ``max_matrix_bytes`` is refused.  Out of
    scope: a matrix-free path for large ``n``, a Boruvka spanning-tree path for single linkage,
    cosine and precomputed affinities, connectivity constraints."""

    def __init__(self, n_clusters=2, metric: str = "euclidean", linkage: str = "ward", distance_threshold=None,
                 use_kernel=None, max_matrix_bytes: int = 1 << 30):
        _check_params(linkage, metric, n_clusters, distance_threshold)
        self.n_clusters = None if n_clusters is None else int(n_clusters)
        self.distance_threshold = None if distance_threshold is None else float(distance_threshold)
        self.metric, self.linkage = metric, linkage
        self.use_kernel, self.max_matrix_bytes = use_kernel, int(max_matrix_bytes)

    def fit(self, X) -> "AgglomerativeClustering":
        if not isinstance(X, torch.Tensor):
            X = torch.from_numpy(np.ascontiguousarray(X))
        _check_shape(tuple(X.shape), X.dtype == torch.float32)
        n = X.shape[0]
        kernel = (X.is_cuda and n >= KERNEL_MIN_ROWS) if self.use_kernel is None else bool(self.use_kernel)
        if kernel and not X.is_cuda:
            raise ValueError("use_kernel=True needs a CUDA tensor")
        _check_cut(n, self.n_clusters)
        _check_bytes(n, self.max_matrix_bytes)
        if kernel:
            res = self._fit_device(X.contiguous())
        else:
            res = agglo_twin(X.detach().cpu().numpy(), self.linkage, self.metric, self.n_clusters,
                             self.distance_threshold, self.max_matrix_bytes)
        self.children_ = torch.from_numpy(res.children).to(X.device)
        self.distances_ = torch.from_numpy(res.distances).to(X.device)
        self.labels_ = torch.from_numpy(res.labels).to(X.device)
        self.rounds_, self.n_leaves_ = res.rounds, n
        self.n_clusters_ = int(res.labels.max()) + 1
        return self

    def fit_predict(self, X) -> torch.Tensor:
        return self.fit(X).labels_

    def _fit_device(self, X: torch.Tensor) -> AggloResult:
        from .. import _native
        C = _native.C()
        if not bool(torch.isfinite(X).all()):
            raise ValueError("X must be finite")
        n = X.shape[0]
        M, top = C.agglo_matrix(X, METRICS[self.metric], _takes_sqrt(self.linkage, self.metric))
        if int(top) > int(ENTRY_LIMIT.view(np.int32)):                # bit order is value order
            raise ValueError("a distance matrix entry exceeds 2**96")
        h, rnd, si, sj, rounds = C.agglo_merge(M, n, LINKAGES[self.linkage])
        del M
        # the sort of n - 1 records and the O(n) relabelling run on the host, as in the twin
        h, rnd, si, sj = (t.cpu().numpy() for t in (h, rnd, si, sj))
        children, distances, si, sj = _dendrogram(n, h, rnd, si, sj, self.linkage)
        labels = _cut(n, si, sj, distances, self.n_clusters, self.distance_threshold)
        return AggloResult(children, distances, labels, int(rounds))
