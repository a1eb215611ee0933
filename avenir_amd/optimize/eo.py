"""Evolutionary optimiser islands: the run record, the launcher, the LDS plans and the host twin of
the K22 island kernels ``eo_assign_kernel`` / ``eo_meeting_kernel`` / ``eo_subset_kernel``
(``csrc/kernels/optim.hip``, frame ``eo_island``); the meeting and subset glue is in :mod:`.ga_meeting` and
:mod:`.ga_subset`.

Reference: ``EvolutionaryOptimizer`` (P/mlextra/optpopu.py:32-92): tournament selection, a mutated
clone, purge by cost and age.  An island's state is

* ``pop``   int16 ``[P, L]``  the pool,
* ``cost``  fp32 ``[P]``      the cost of each member,
* ``born``  int32 ``[P]``     insertion stamps, distinct; initial member ``j`` has stamp ``j``,
* ``best``  int16 ``[L]``     the best solution seen, ``best_cost`` fp32 its cost (where none is passed
  in: the first smallest-cost member).

Island ``g = island_base + i`` is GLOBAL.  Iteration ``it`` of ``[it_begin, it_begin + iters)``, every
fp32 operation rounded on its own:

1. *Tournament.*  ``k = select`` distinct slots are drawn.  Draw ``j = 0..k-1`` takes
   ``t = min(int(u_j * float32(P - j)), P - j - 1)`` and picks the ``t``-th slot, slots ascending, that
   no earlier draw picked; ``u_j`` is word ``j & 3`` of ``Philox(seed ^ EO_SEL_KEY, 16 it + (j >> 2), g)``.
   The winner is the picked slot of smallest cost, ties to the earlier draw (the reference's
   ``findBest`` keeps the first).
2. *Clone and mutate.*  Attempt ``t = 0..EO_MAX_TRY-1`` (5, the reference's ``maxTry``) draws
   ``Philox(seed ^ GA_MUT_KEY, 16 it + t, g)``: word x picks the position, word y the value, and the
   domain's mutation (the one of its island GA kernel) is applied to the clone.  An attempt that
   leaves the whole clone invalid is taken back; the first valid attempt is the child.  Without one
   the iteration inserts nothing and counts in ``stalls`` (the reference raises).
3. *Price.*  The child is priced from scratch by the domain's price function.
4. *Purge.*  ``a_j`` is the number of members whose stamp is older than member ``j``'s,
   ``age_j = (float32(P - a_j) * age_scale) / float32(P)``, ``fin_j`` is ``cost_j`` when finite, else
   ``1e30``, ``aggr_j = w * fin_j + (1 - w) * age_j``.  The victim has the largest ``aggr``, ties to the
   oldest.  The child takes the victim's slot with stamp ``P + it``; ``inserted`` counts.
5. *Best.*  A child cost strictly below ``best_cost`` replaces the best (``improved``);
   ``hist[i, it - it_begin]`` is the island's best cost after the iteration.

Limits: ``2 <= P <= 64``, ``1 <= select <= P``, ``0 <= w <= 1``, ``it_begin + iters + P < 2^31``.  A
run cut into segments through the returned state equals one run, and the kernels equal
:func:`eo_islands_reference` bit for bit.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable

import numpy as np
import torch

from ..ops.random import philox4x32, u32_to_unit
from .ga import _MUT_KEY, GaDomain, ga_assign_domain

EO_SEL_KEY = 0xA0761D6478BD642F      # the kernels' tournament stream key (seed ^ this)
EO_MAX_TRY = 5
LDS_LIMIT = 64 * 1024                # bytes of LDS a workgroup (one wave) of the kernels may take
_DOM_INTS = 3 * 32 + 2 * 32 + 2 * 256 + 5 * 16      # the staged meeting domain (optim.hip MT_DOM_INTS)
_F = np.float32
_COUNTERS = ("inserted", "stalls", "improved")


@dataclass(frozen=True)
class EoRun:
    """Iterations ``[it_begin, it_begin + iters)`` of islands ``island_base ..``, the mirror of
    ``avk::EoRun``: tournaments of ``select`` members, purge by ``w * cost + (1 - w) * age``."""
    iters: int
    select: int
    w: float = 0.7
    age_scale: float = 1.0
    seed: int = 0
    it_begin: int = 0
    island_base: int = 0


def eo_pool_ok(P: int, select: int, w: float, age_scale: float, iters: int, it_begin: int = 0) -> bool:
    """The limits of the frame (``eo_args`` in optim.hip)."""
    return (2 <= P <= 64 and 1 <= select <= P and 0.0 <= w <= 1.0 and 0.0 <= age_scale < float("inf")
            and iters >= 0 and it_begin >= 0 and it_begin + iters + P < 2 ** 31)


def _plan(per: int, shared: int) -> tuple[int, int]:
    for iw in (64, 32, 16, 8, 4, 2, 1):
        if shared + iw * per <= LDS_LIMIT:
            return iw, shared + iw * per
    return 0, shared + per


def eo_island_bytes(P: int, L: int, M: int = 0) -> int:
    """Bytes of one island's lane-private LDS columns: fp32 costs (4 P), for meetings the clone's start
    seconds and day bits (8 M), int16 age ranks (2 P), the int16 pool (2 P L) and the clone (2 L)."""
    return 4 * P + 8 * M + 2 * P + 2 * P * L + 2 * L


def eo_assign_plan(P: int, L: int) -> tuple[int, int]:
    """(islands per wave IW, LDS bytes per workgroup) of ``eo_assign_kernel`` (``avk::eo_assign_plan``): IW
    is the largest of 64, 32, ..., 1 with ``IW * eo_island_bytes(P, L) <= 64 KiB``; ``IW = 0`` means
    that one island does not fit and there is no kernel."""
    return _plan(eo_island_bytes(P, L), 0)


def eo_meeting_plan(P: int, M: int) -> tuple[int, int]:
    """The same for ``eo_meeting_kernel``: the staged domain (3,008 bytes) in front of the columns."""
    return _plan(eo_island_bytes(P, 3 * M, M), 4 * _DOM_INTS)


def _check_state(P: int, born: np.ndarray, run: EoRun) -> None:
    if not eo_pool_ok(P, run.select, run.w, run.age_scale, run.iters, run.it_begin):
        raise ValueError("eo: 2 <= P <= 64, 1 <= select <= P, 0 <= w <= 1, 0 <= age_scale < inf and "
                         "0 <= iters, it_begin with it_begin + iters + P < 2^31")
    if born.size:
        s = np.sort(born, axis=1)
        if (s[:, 1:] == s[:, :-1]).any():
            raise ValueError("eo: the insertion stamps of an island must be distinct")


def eo_islands_reference(dom: GaDomain, pop, cost, run: EoRun, born=None, best=None, best_cost=None,
                         trace: dict | None = None):
    """Host twin of optim.hip's ``eo_island``, vectorised over the islands (the leading axis of ``pop``)
    and driven by a :class:`~avenir_amd.optimize.ga.GaDomain` (its ``encode / decode / mutated / valid /
    price``).  Returns (best int16, best_cost, stats, pop int16, cost, born int32, hist): ``stats`` is
    ``inserted`` / ``stalls`` / ``improved`` summed over the islands, ``hist [I, iters]`` the best cost
    after every iteration.  ``trace``, when given, collects what the counters do not show:
    ``tied`` (tournaments whose smallest cost two picked members share), ``winner`` and ``victim``
    (``[I, iters]`` slots, -1 without an insert) and ``picked`` (``[I, P]`` tournament picks per slot)."""
    pool = dom.encode(np.asarray(pop))
    pc = np.array(cost, dtype=np.float32)
    I, P = pool.shape[:2]
    born = (np.broadcast_to(np.arange(P, dtype=np.int32), (I, P)).copy() if born is None
            else np.array(born, dtype=np.int32))
    _check_state(P, born, run)
    ar = np.arange(I)
    if best_cost is None:
        first = pc.argmin(1) if I else np.zeros(0, dtype=np.int64)
        bsol, bc = pool[ar, first].copy(), pc[ar, first].copy()
    else:
        bsol = dom.encode(np.asarray(best)[:, None])[:, 0].copy()
        bc = np.array(best_cost, dtype=np.float32)
    iters, k = max(int(run.iters), 0), int(run.select)
    hist = np.empty((I, iters), dtype=np.float32)
    gis = np.arange(run.island_base, run.island_base + I, dtype=np.uint64)
    w, scale, Pf = _F(run.w), _F(run.age_scale), _F(P)
    wa = _F(1.0) - w
    st = [0, 0, 0]
    if trace is not None:
        trace.update(tied=0, winner=np.full((I, iters), -1), victim=np.full((I, iters), -1),
                     picked=np.zeros((I, P), dtype=np.int64))
    for n in range(iters):
        it = run.it_begin + n
        # 1. tournament
        free = np.ones((I, P), dtype=bool)
        win = np.zeros(I, dtype=np.int64)
        wc = np.zeros(I, dtype=np.float32)
        tie = np.zeros(I, dtype=bool)
        for j in range(k):
            if j & 3 == 0:
                words = philox4x32(run.seed ^ EO_SEL_KEY, 16 * it + (j >> 2), gis)
            left = P - j
            t = np.minimum((u32_to_unit(words[j & 3]) * _F(left)).astype(np.int64), left - 1)
            slot = ((np.cumsum(free, axis=1) == (t + 1)[:, None]) & free).argmax(1)
            free[ar, slot] = False
            c = pc[ar, slot]
            take = np.full(I, True) if j == 0 else c < wc
            tie = np.where(take, False, tie | (c == wc))
            win = np.where(take, slot, win)
            wc = np.where(take, c, wc)
            if trace is not None:
                trace["picked"][ar, slot] += 1
        # 2. clone and mutate
        child = pool[ar, win].copy()
        done = np.zeros(I, dtype=bool)
        for t in range(EO_MAX_TRY):
            todo = np.nonzero(~done)[0]
            if todo.size == 0:
                break
            q = philox4x32(run.seed ^ _MUT_KEY, 16 * it + t, gis[todo])
            cand = dom.mutated(child[todo], q[0], q[1])
            ok = dom.valid(cand)
            child[todo[ok]] = cand[ok]
            done[todo[ok]] = True
        ins = np.nonzero(done)[0]
        st[0] += int(ins.size)
        st[1] += int(I - ins.size)
        if ins.size:
            # 3. price
            cc = np.asarray(dom.price(child[ins]), dtype=np.float32)
            # 4. purge
            a = (born[ins][:, None, :] < born[ins][:, :, None]).sum(-1)
            with np.errstate(over="ignore"):
                age = ((P - a).astype(np.float32) * scale) / Pf
                fin = np.where(np.isfinite(pc[ins]), pc[ins], _F(1e30)).astype(np.float32)
                aggr = w * fin + wa * age
            top = aggr == aggr.max(1, keepdims=True)
            vic = np.where(top, a, P).argmin(1)
            pool[ins, vic] = child[ins]
            pc[ins, vic] = cc
            born[ins, vic] = P + it
            # 5. best
            imp = cc < bc[ins]
            bsol[ins[imp]] = child[ins[imp]]
            bc[ins[imp]] = cc[imp]
            st[2] += int(imp.sum())
            if trace is not None:
                trace["winner"][ins, n] = win[ins]
                trace["victim"][ins, n] = vic
        if trace is not None:
            trace["tied"] += int(tie.sum())
        hist[:, n] = bc
    out_best = dom.decode(bsol[:, None])[:, 0]
    return out_best, bc, dict(zip(_COUNTERS, st)), dom.decode(pool), pc, born, hist


def eo_islands_launch(kernel: Callable, head: tuple, pop, cost, run: EoRun, born=None, best=None, best_cost=None,
                      device=None):
    """One launch of a native island kernel, ``kernel(*head, pop, pop_cost, born, best, best_cost, hist,
    iters, select, w, age_scale, seed, it_begin, island_base, stats)``, on private device copies of the
    state: numpy (to ``device`` and back) or tensors that are already on the GPU (the results stay
    there).  Returns what :func:`eo_islands_reference` returns."""
    resident = isinstance(pop, torch.Tensor)
    if resident and not pop.is_cuda:
        raise ValueError("eo_islands_launch takes numpy state, or tensors that are already on the GPU")

    def own(x, dtype):
        if resident:
            return x.to(dtype=getattr(torch, np.dtype(dtype).name), copy=True).contiguous()
        return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(device)

    p16, pc = own(pop, np.int16), own(cost, np.float32)
    I, P = p16.shape[:2]
    dev = p16.device
    tb = (torch.arange(P, dtype=torch.int32, device=dev).repeat(I, 1) if born is None else own(born, np.int32))
    _check_state(P, tb.cpu().numpy(), run)
    if best_cost is None:
        first = pc.argmin(1) if I else torch.zeros(0, dtype=torch.long, device=dev)
        ii = torch.arange(I, device=dev)
        bsol, bc = p16[ii, first].contiguous(), pc[ii, first].contiguous()
    else:
        bsol, bc = own(best, np.int16), own(best_cost, np.float32)
    hist = torch.empty((I, max(int(run.iters), 0)), dtype=torch.float32, device=dev)
    st = torch.zeros(4, dtype=torch.long, device=dev)
    kernel(*head, p16, pc, tb, bsol, bc, hist, int(run.iters), int(run.select), float(run.w), float(run.age_scale),
           int(run.seed), int(run.it_begin), int(run.island_base), st)
    n = st.tolist()
    out = (bsol, bc, p16, pc, tb, hist)
    if not resident:
        out = tuple(x.cpu().numpy() for x in out)
    return out[0], out[1], dict(zip(_COUNTERS, n[:3])), out[2], out[3], out[4], out[5]


def _numpy_state(*xs):
    return [None if x is None else (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x) for x in xs]


# ---- assignment domains (optim.hip::eo_assign_kernel) --------------------------------------------------
def eo_assign_advance(d, pop, cost, run: EoRun, device, born=None, best=None, best_cost=None):
    """One segment over AssignmentDomain ``d``: ``eo_assign_kernel`` on a GPU, the twin otherwise — the
    frame with the mutation of ``ga_assign_kernel`` (swap move included), ``ga_valid`` and ``ga_price``.
    The kernel indexes the cost table with solution values; the binding checks them once per call."""
    if torch.device(device).type == "cuda":
        from .. import _native
        dev = torch.device(device)
        cf = None if d.conflict is None else d.conflict.to(device=dev, dtype=torch.uint8).contiguous()
        head = (d.cost_table.to(dev).float().contiguous(), cf, bool(d.swap_moves))
        return eo_islands_launch(_native.C().eo_assign, head, pop, cost, run, born, best, best_cost, dev)
    pop, cost, born, best, best_cost = _numpy_state(pop, cost, born, best, best_cost)
    for s in (pop, best):
        if s is not None and np.size(s) and (np.min(s) < 0 or np.max(s) >= d.V):
            raise ValueError(f"eo_assign: solution values must lie in [0, {d.V})")
    conf = None if d.conflict is None else d.conflict.cpu().numpy()
    dom = ga_assign_domain(d.cost_table.cpu().numpy(), conf, d.invalid_cost, bool(d.swap_moves))
    return eo_islands_reference(dom, pop, cost, run, born, best, best_cost)


def eo_assign_reference(d, pop, cost, run: EoRun, born=None, best=None, best_cost=None, trace: dict | None = None):
    """Host twin of ``eo_assign_kernel`` over AssignmentDomain ``d`` (:func:`eo_islands_reference`)."""
    conf = None if d.conflict is None else d.conflict.cpu().numpy()
    dom = ga_assign_domain(d.cost_table.cpu().numpy(), conf, d.invalid_cost, bool(d.swap_moves))
    return eo_islands_reference(dom, pop, cost, run, born, best, best_cost, trace)
