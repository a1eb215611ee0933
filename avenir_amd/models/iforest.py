"""The deterministic isolation forest: its numeric contract, the numpy twin that defines it, and the
dispatch onto the device kernels (csrc/kernels/iforest.hip).

``models/outlier.py::IsolationForest(engine="philox")`` runs this.  Every draw is Philox4x32-10
(``avenir_common.h::philox4x32_10``, twinned by ``ops/random.py::philox4x32``), so the forest is a
pure function of ``(X, n_trees, psi, seed, tree_base)``: no grid, launch split or device enters it,
and the kernels equal the twin bit for bit.

Layout (that of ``models/outlier.py``): depth ``L = max(1, ceil(log2(max(psi, 2))))``, heap-indexed
complete trees of ``M = 2^(L+1) - 1`` nodes, ``feat [T, M]`` int32 (-1 at leaves and unreached
nodes), ``thr [T, M]`` fp32 (0 there), ``size [T, M]`` int32 (rows that reached the node).

* **Sample of tree** ``g = tree_base + t``: ``psi`` distinct rows by Floyd's algorithm.  For
  ``s = 0 .. psi-1``: ``j = n - psi + s``, ``r = (x * (j + 1)) >> 32`` with ``x`` word 0 of
  ``philox(key = seed ^ SAMPLE_KEY, offset = g, idx = s)``; slot ``s`` takes ``r``, or ``j`` if ``r``
  is already taken.  ``n < 2^31``.
* **Split at heap node** ``i``: fp32 min / max of every feature over the node's rows; the varying
  features are those with ``max > min``, ``nv`` of them in ascending order; with ``(x, y, ., .) =
  philox(key = seed ^ NODE_KEY, offset = g, idx = i)`` the split feature is the
  ``((x * nv) >> 32)``-th varying one.  A node with no varying feature, or at depth ``L``, is a leaf.
* **Threshold**: ``u = float(y >> 8) * 2^-24``, ``thr = lo + u * (hi - lo)`` with the multiply and the
  add rounded separately; ``thr = lo`` unless ``thr < hi`` (which also catches an overflowing
  ``hi - lo``).  A row goes to ``2i + 2`` iff ``x[f] > thr``, else to ``2i + 1``; both are non-empty.
* **Path length** of a row: for ``t`` ascending ``acc = acc + (float(depth_t) + leaf_c[t, leaf])`` in
  fp32, every operation rounded on its own; the result is ``acc / float(T)``.  ``leaf_c`` is
  ``float32(c(size))`` with ``c`` in fp64 (``outlier.avg_path_length``), always computed on the host.

Everything a tree stores is a count, a minimum or a maximum, so no reduction order is part of the
contract.  X must be finite.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ..ops.random import philox4x32

SAMPLE_KEY = 0x9E6C63D0876A9A47
NODE_KEY = 0xB5AD4ECEDA1CE2A9
_MASK64 = (1 << 64) - 1

# limits of the kernels (iforest.hip); beyond them a CUDA input runs the twin on a host copy
KERNEL_MAX_PSI = 1024
KERNEL_MAX_D = 64
MAX_ROWS = 1 << 31


def iforest_depth(psi: int) -> int:
    return max(1, math.ceil(math.log2(max(int(psi), 2))))


def _tree_ids(n_trees: int, tree_base: int) -> np.ndarray:
    return (np.arange(n_trees, dtype=np.uint64) + np.uint64(int(tree_base) & _MASK64))


def _check(n: int, psi: int, n_trees: int):
    if not 1 <= psi <= n:
        raise ValueError("psi must lie in 1 .. n")
    if n >= MAX_ROWS:
        raise ValueError("the isolation forest takes fewer than 2^31 rows")
    if n_trees < 1:
        raise ValueError("n_trees must be at least 1")


def iforest_sample(n: int, psi: int, n_trees: int, seed: int, tree_base: int = 0) -> np.ndarray:
    """The sampled rows of every tree, int64 [T, psi], in Floyd's slot order."""
    _check(n, psi, n_trees)
    g = _tree_ids(n_trees, tree_base)
    key = (int(seed) ^ SAMPLE_KEY) & _MASK64
    out = np.empty((n_trees, psi), dtype=np.int64)
    for s in range(psi):
        j = n - psi + s
        x = philox4x32(key, g, np.full(n_trees, s, dtype=np.uint64))[0]
        r = ((x.astype(np.uint64) * np.uint64(j + 1)) >> np.uint64(32)).astype(np.int64)
        taken = (out[:, :s] == r[:, None]).any(1)
        out[:, s] = np.where(taken, j, r)
    return out


def iforest_build_twin(X, n_trees: int, psi: int, seed: int, tree_base: int = 0):
    """``feat`` int32, ``thr`` fp32, ``size`` int32, each [T, M], by the definition above."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    if X.ndim != 2 or X.shape[1] < 1:
        raise ValueError("X must be [n, D >= 1]")
    n, D = X.shape
    T = int(n_trees)
    idx = iforest_sample(n, psi, T, seed, tree_base)
    L = iforest_depth(psi)
    M = (1 << (L + 1)) - 1
    S = X[idx]                                                        # [T, psi, D]
    feat = np.full((T, M), -1, dtype=np.int32)
    thr = np.zeros((T, M), dtype=np.float32)
    size = np.zeros((T, M), dtype=np.int32)
    node = np.zeros((T, psi), dtype=np.int64)
    g = _tree_ids(T, tree_base)
    key = (int(seed) ^ NODE_KEY) & _MASK64
    for lev in range(L + 1):
        base, width = (1 << lev) - 1, 1 << lev
        tr, sl = np.nonzero(node >= base)                             # rows whose node is on this level
        if tr.size == 0:
            break
        cur = node[tr, sl]
        flat = tr * width + (cur - base)
        size[:, base:base + width] = np.bincount(flat, minlength=T * width).reshape(T, width)
        if lev == L:
            break
        order = np.argsort(flat, kind="stable")
        fs = flat[order]
        rows = S[tr[order], sl[order]]
        starts = np.flatnonzero(np.r_[True, fs[1:] != fs[:-1]])
        ids = fs[starts]                                              # the nodes that hold rows
        mn = np.minimum.reduceat(rows, starts, axis=0)
        mx = np.maximum.reduceat(rows, starts, axis=0)
        varies = mx > mn
        nv = varies.sum(1)
        t_of, heap = ids // width, base + ids % width
        x, y, _, _ = philox4x32(key, g[t_of], heap.astype(np.uint64))
        k = (x.astype(np.uint64) * nv.astype(np.uint64)) >> np.uint64(32)
        f = np.argmax(varies & (np.cumsum(varies, 1) == (k.astype(np.int64) + 1)[:, None]), axis=1)
        ar = np.arange(ids.size)
        lo, hi = mn[ar, f], mx[ar, f]
        u = (y >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        with np.errstate(over="ignore", invalid="ignore"):
            th = lo + u * (hi - lo)
        th = np.where(th < hi, th, lo)
        sp = nv > 0
        feat[t_of[sp], heap[sp]] = f[sp]
        thr[t_of[sp], heap[sp]] = th[sp]
        nf = feat[tr, cur]
        go = nf >= 0
        right = S[tr, sl, np.maximum(nf, 0)] > thr[tr, cur]
        node[tr[go], sl[go]] = (2 * cur + 1 + right)[go]
    return feat, thr, size


def leaf_c_table(size) -> np.ndarray:
    """``float32(c(size))`` of every node, c in fp64 as ``outlier.avg_path_length`` computes it."""
    from .outlier import avg_path_length
    return avg_path_length(torch.from_numpy(np.ascontiguousarray(size))).float().numpy()


def iforest_path_twin(X, feat, thr, leaf_c, chunk: int = 1 << 13) -> np.ndarray:
    """The mean path length of every row of X, fp32 [n], by the definition above."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    feat, thr, leaf_c = np.asarray(feat), np.asarray(thr, dtype=np.float32), np.asarray(leaf_c, dtype=np.float32)
    T, M = feat.shape
    L = int(M + 1).bit_length() - 2
    if (1 << (L + 1)) - 1 != M or L < 1:
        raise ValueError("feat must be [T, 2^(L+1) - 1]")
    if feat.min(initial=-1) < -1 or feat.max(initial=-1) >= X.shape[1]:
        raise ValueError("feat outside [-1, D)")
    out = np.empty(X.shape[0], dtype=np.float32)
    tcol = np.arange(T)[:, None]
    for s in range(0, X.shape[0], chunk):
        xc = X[s:s + chunk]
        col = np.arange(xc.shape[0])[None, :]
        node = np.zeros((T, xc.shape[0]), dtype=np.int64)
        depth = np.zeros((T, xc.shape[0]), dtype=np.int32)
        for _ in range(L):
            f = feat[tcol, node]
            inner = f >= 0
            right = xc[col, np.maximum(f, 0)] > thr[tcol, node]
            node = np.where(inner, 2 * node + 1 + right, node)
            depth += inner
        term = depth.astype(np.float32) + leaf_c[tcol, node]
        acc = np.zeros(xc.shape[0], dtype=np.float32)
        for t in range(T):
            acc = acc + term[t]
        out[s:s + chunk] = acc / np.float32(T)
    return out


def kernel_supports(psi: int, D: int) -> bool:
    return 1 <= psi <= KERNEL_MAX_PSI and 1 <= D <= KERNEL_MAX_D


def use_kernel_for(X: torch.Tensor, psi: int, use_kernel) -> bool:
    """The dispatch of ``engine="philox"``: the kernels for a CUDA tensor within their limits, else
    the twin (on a host copy of a CUDA tensor).  ``use_kernel=True`` insists and raises otherwise."""
    ok = kernel_supports(psi, X.shape[1])
    if use_kernel is None:
        return X.is_cuda and ok
    if use_kernel:
        if not X.is_cuda:
            raise ValueError("use_kernel=True needs a CUDA tensor")
        if not ok:
            raise ValueError(f"use_kernel=True: the kernels take psi <= {KERNEL_MAX_PSI} and D <= {KERNEL_MAX_D}")
    return bool(use_kernel)


def build(X: torch.Tensor, n_trees: int, psi: int, seed: int, tree_base: int, use_kernel):
    """``feat``, ``thr``, ``size`` and ``leaf_c`` as tensors on the device of X (fp32 [n, D], finite)."""
    _check(X.shape[0], psi, n_trees)
    if not bool(torch.isfinite(X).all()):
        raise ValueError("X must be finite")
    if use_kernel_for(X, psi, use_kernel):
        from .. import _native
        feat, thr, size = _native.C().iforest_build(X.contiguous(), int(n_trees), int(psi), int(seed) & _MASK64,
                                                    int(tree_base) & _MASK64)
    else:
        feat, thr, size = (torch.from_numpy(a).to(X.device) for a in
                           iforest_build_twin(X.detach().cpu().numpy(), n_trees, psi, seed, tree_base))
    leaf_c = torch.from_numpy(leaf_c_table(size.cpu().numpy())).to(X.device)
    return feat, thr, size, leaf_c


def path_length(X: torch.Tensor, feat, thr, leaf_c, psi: int, use_kernel) -> torch.Tensor:
    if use_kernel_for(X, psi, use_kernel):
        from .. import _native
        return _native.C().iforest_score(X.contiguous(), feat, thr, leaf_c)
    out = iforest_path_twin(X.detach().cpu().numpy(), feat.cpu().numpy(), thr.cpu().numpy(), leaf_c.cpu().numpy())
    return torch.from_numpy(out).to(X.device)
