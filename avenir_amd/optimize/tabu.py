"""Tabu search over assignment domains: the run record, the launcher and the host twin of the K22
kernel ``tabu_assign_kernel`` (``csrc/kernels/optim.hip``).

Reference: the tenure purge of ``TabuSearchDomain`` (J/optimize/TabuSearchDomain.java:54-66) over the
single-reassignment neighbourhood of an :class:`~avenir_amd.optimize.domain.AssignmentDomain`.  The
state of a chain is its solution ``sol [L]``, the solution's ``cost``, the best solution and its cost,
and the table ``tabu [L, V]`` int32: ``tabu[l, v]`` is the first iteration at which moving position
``l`` to value ``v`` is free again (a fresh table is all -1).  Iteration ``it`` of ``[it_begin,
it_begin + iters)``, with ``C`` the fp32 cost table:

1. every cell ``(l, v)`` is priced ``nc = cost + ((C[l, v] - C[l, sol[l]]) / float32(L))``: the
   difference, the IEEE division and the sum are each rounded to fp32 on their own;
2. a cell is bad when ``v == sol[l]`` or some ``j != l`` has ``conflict[l, j]`` and ``sol[j] == v``
   (no swap moves: the neighbourhood of ``AssignmentDomain.neighbourhood_delta``);
3. a cell is admissible when it is not bad and (``tabu[l, v] <= it`` or ``nc < best_cost``, the
   aspiration, against the best cost at the iteration's start);
4. the move is the admissible cell of smallest ``nc``, ties to the smallest ``l V + v``, taken only
   if ``nc < +inf``; the comparisons are float comparisons (-0.0 == 0.0, a NaN never wins);
5. a move sets ``tabu[l, sol[l]] = it + tenure``, ``sol[l] = v`` and ``cost = nc`` and counts in
   ``moves`` (and in ``aspirated`` when the cell was tabu); without one ``stalls`` counts;
6. a cost below the best replaces the best;
7. ``hist[p, it - it_begin]`` is the best cost.

The algorithm is deterministic after the start solutions, so the kernel equals
:func:`tabu_assign_reference` bit for bit, and a run cut into segments through the returned state
(the table included) equals one run.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

# Bytes of LDS a workgroup of tabu_assign_kernel may take.  It is the only limit of the default
# dispatch: one chain is one wave, so a run's time grows with L V / 64 whatever the chain count, but
# at 16 chains the kernel stayed 8.6 to 54 times faster than the generic path for every size of
# profiles/tabu_assign_cap_sweep.jsonl, 24 x 10 to 100 x 100 cells (benchmarks/bench_tabu_assign.py).
LDS_LIMIT = 64 * 1024


@dataclass(frozen=True)
class TabuRun:
    """Iterations ``[it_begin, it_begin + iters)`` of chains ``chain_base ..``; reversing a move is
    tabu for ``tenure`` iterations."""
    iters: int
    tenure: int
    it_begin: int = 0
    chain_base: int = 0


def _a16(n: int) -> int:
    return (n + 15) & ~15


def tabu_assign_plan(L: int, V: int) -> tuple[int, bool, int]:
    """(waves per workgroup, tables staged, LDS bytes) of the launcher (``avk::tabu_assign_plan``).  A
    chain keeps its tabu table (int32), the blocked counts (uint16), its solution and the cost of
    each position's value in LDS; the 4, 2 or 1 chains of a workgroup share one copy of the cost
    table and the transposed conflict table when those fit beside them, else one chain per
    workgroup reads both from global memory."""
    LV = L * V
    per = _a16(4 * LV) + _a16(4 * L) + _a16(2 * LV) + _a16(2 * L)
    shared = _a16(4 * LV) + _a16(L * L)
    for w in (4, 2, 1):
        if w * per + shared <= LDS_LIMIT:
            return w, True, w * per + shared
    return 1, False, per


def tabu_assign_lds(L: int, V: int) -> int:
    """Bytes of LDS per workgroup the launcher asks for; above ``LDS_LIMIT`` there is no kernel."""
    return tabu_assign_plan(L, V)[2]


def tabu_assign_reference(cost_table, conflict, sol, cost, run: TabuRun, tabu=None, best=None, best_cost=None):
    """Host twin of ``tabu_assign_kernel``, vectorised over the chains (the leading axis of ``sol``).
    Returns (best, best_cost, stats, sol, cost, tabu, hist): ``stats`` is ``moves`` / ``stalls`` /
    ``aspirated`` summed over the chains, ``hist [P, iters]`` the best cost after every iteration."""
    C = np.ascontiguousarray(cost_table, dtype=np.float32)
    L, V = C.shape
    sol = np.array(sol, dtype=np.int64)
    P = sol.shape[0]
    c = np.array(cost, dtype=np.float32)
    bc = c.copy() if best_cost is None else np.array(best_cost, dtype=np.float32)
    best = sol.copy() if best is None else np.array(best, dtype=np.int64)
    tabu = np.full((P, L, V), -1, dtype=np.int32) if tabu is None else np.array(tabu, dtype=np.int32)
    hist = np.empty((P, max(run.iters, 0)), dtype=np.float32)
    conf = None
    if conflict is not None:
        conf = (np.asarray(conflict) != 0) & ~np.eye(L, dtype=bool)
        conf = conf.astype(np.int32)
    rows, ar, vals = np.arange(P), np.arange(L), np.arange(V)
    Lf = np.float32(L)
    inf = np.float32(np.inf)
    st = [0, 0, 0]
    for k in range(run.iters):
        it = run.it_begin + k
        cur = C[ar[None, :], sol]                                             # [P, L]
        with np.errstate(invalid="ignore", over="ignore"):
            d = (C[None, :, :] - cur[:, :, None]).astype(np.float32)          # step 1: three roundings
            d = (d / Lf).astype(np.float32)
            nc = (c[:, None, None] + d).astype(np.float32)
        occ = sol[:, :, None] == vals[None, None, :]                          # [P, L, V]
        bad = occ if conf is None else occ | (np.matmul(conf[None], occ.astype(np.int32)) > 0)
        was_tabu = tabu > it
        adm = ~bad & (~was_tabu | (nc < bc[:, None, None])) & (nc < inf)      # a NaN is never < inf
        score = np.where(adm, nc, inf).reshape(P, L * V)
        flat = score.argmin(1)                                                # the first of the smallest
        has = score[rows, flat] < inf
        h = rows[has]
        l, v = flat[has] // V, flat[has] % V
        old = sol[h, l]
        st[0] += int(h.size)
        st[1] += int(P - h.size)
        st[2] += int(was_tabu[h, l, v].sum())
        tabu[h, l, old] = it + run.tenure
        sol[h, l] = v
        c[h] = score[h, flat[has]]
        imp = c < bc
        best[imp] = sol[imp]
        bc[imp] = c[imp]
        hist[:, k] = bc
    return best, bc, {"moves": st[0], "stalls": st[1], "aspirated": st[2]}, sol, c, tabu, hist


def tabu_assign_advance(d, sol, cost, run: TabuRun, device, tabu=None, best=None, best_cost=None):
    """One segment over AssignmentDomain ``d``: ``tabu_assign_kernel`` on a GPU, the twin otherwise, with
    the twin's return.  The state is numpy (to ``device`` and back) or tensors that are already on
    the GPU (the results stay there).  Every solution value must lie in ``[0, V)``: the kernel
    indexes its LDS tables with them, so the launcher checks that once per call."""
    L, V = d.L, d.V
    if torch.device(device).type != "cuda":
        state = [None if x is None else (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x)
                 for x in (sol, cost, tabu, best, best_cost)]
        s = np.asarray(state[0])
        if s.size and (s.min() < 0 or s.max() >= V):
            raise ValueError(f"tabu_assign: solution values must lie in [0, {V})")
        conf = None if d.conflict is None else d.conflict.cpu().numpy()
        return tabu_assign_reference(d.cost_table.cpu().numpy(), conf, state[0], state[1], run, *state[2:])
    from .. import _native
    resident = isinstance(sol, torch.Tensor)
    if resident and not sol.is_cuda:
        raise ValueError("tabu_assign_advance takes numpy state, or tensors that are already on the GPU")

    def own(x, dtype):
        if resident:
            return x.to(dtype=getattr(torch, np.dtype(dtype).name), copy=True).contiguous()
        return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(device)

    s16, cur = own(sol, np.int16), own(cost, np.float32)
    P = s16.shape[0]
    if s16.numel() and bool(((s16 < 0) | (s16 >= V)).any()):
        raise ValueError(f"tabu_assign: solution values must lie in [0, {V})")
    bsol = s16.clone() if best is None else own(best, np.int16)
    bc = cur.clone() if best_cost is None else own(best_cost, np.float32)
    tb = (torch.full((P, L, V), -1, dtype=torch.int32, device=s16.device) if tabu is None else own(tabu, np.int32))
    hist = torch.empty((P, max(int(run.iters), 0)), dtype=torch.float32, device=s16.device)
    st = torch.zeros(4, dtype=torch.long, device=s16.device)
    conf = None if d.conflict is None else d.conflict.to(device=s16.device, dtype=torch.uint8).contiguous()
    _native.C().tabu_assign(d.cost_table.to(s16.device), conf, s16, cur, bsol, bc, tb, hist, int(run.iters),
                            int(run.tenure), int(run.it_begin), st)
    n = st.tolist()
    out = (bsol, bc, s16, cur, tb, hist)
    if not resident:
        out = tuple(x.cpu().numpy() for x in out)
    return out[0], out[1], {"moves": n[0], "stalls": n[1], "aspirated": n[2]}, out[2], out[3], out[4], out[5]
