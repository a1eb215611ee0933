"""Simulated-annealing chains: the run record, the launcher and the host twins of the K22 chain
kernels (``csrc/kernels/optim.hip``) — ``sa_chain`` with ``sa_meeting_kernel`` and ``sa_subset_kernel``
over any domain, bit-exact, and ``sa_assign_kernel`` over assignment domains (at the end).

Reference: the Spark ``simulatedAnnealing`` job (S/optimize/SimulatedAnnealing.scala:111-187) and the
Python ``SimulatedAnnealingOptimizer`` (P/mlextra/optsolo.py:34-88, driven by ``fesel sa``).  A chain
is keyed by its GLOBAL index ``g = chain_base + p``; move ``it`` of ``[it_begin, it_begin + iters)``:

1. attempts ``tr = 0..max_retry`` draw ``Philox(seed, offset + it (max_retry + 1) + tr, g)``: word x
   picks the position, word y the value.  The first attempt that gives a valid candidate is the move;
   without one nothing happens and no counter changes;
2. the candidate is priced from scratch, so the current cost is always the price of the solution;
3. ``cc <= c`` is accepted (``better``; this covers ``c = inf``), otherwise
   ``u(Philox(seed ^ 0x9E3779B97F4A7C15, offset + it, g).x) < sa_exp(-((cc - c) / max(temp, 1e-12)))``
   is accepted (``worse_accepted``), and the rest is ``rejected``;
4. on acceptance the candidate becomes the solution, and a cost below the best replaces the best;
5. cooling after every move when ``interval > 0 and (it + 1) % interval == 0``: ``temp * cool``, or
   ``max(t0 - float32(it + 1) * cool, 1e-12)``.

Everything is fp32 with each operation rounded on its own, and :func:`sa_exp` is built from such
operations alone, so the kernels equal :func:`sa_chains_reference` bit for bit — the Metropolis
decision included.  What a solution is, when it is valid and what it costs is the domain's
(:class:`SaDomain`); :mod:`.ga_meeting` and :mod:`.ga_subset` supply the two of the kernels.
"""
from __future__ import annotations

from dataclasses import astuple, dataclass
from typing import Callable

import numpy as np
import torch

from ..ops.random import philox4x32, u32_to_unit
from .ga import ga_redraw_init

_ACCEPT_KEY = 0x9E3779B97F4A7C15   # the acceptance stream (seed ^ this), as sa_assign_kernel
_F = np.float32
_LOG2E, _LN2_HI, _LN2_LO = _F(1.4426950408889634), _F(0.693359375), _F(-2.12194440e-4)
# 1/720 .. 1: the Taylor coefficients, each one fp32 division as the kernel's constants
_TAYLOR = tuple(_F(1.0) / _F(d) for d in (720.0, 120.0, 24.0, 6.0, 2.0, 1.0, 1.0))
_T_MIN = _F(1e-12)


def sa_exp(x) -> np.ndarray:
    """``exp(x)`` for ``x <= 0`` in fp32, the twin of optim.hip's ``sa_exp``: x clamped to -87 (the
    result stays a normal number), ``k = rint(x log2 e)``, the reduction ``r = (x - k LN2_HI) - k LN2_LO``
    (LN2_HI = 355 / 512, so the first product is exact), the degree-6 Taylor polynomial by Horner
    with product and sum rounded separately, and the exact scaling by ``2^k``.  Within 1e-6 relative
    of float64 ``exp`` (tests/test_sa_meeting.py)."""
    x = np.maximum(np.asarray(x, dtype=np.float32), _F(-87.0))
    k = np.rint(x * _LOG2E)
    r = x - k * _LN2_HI
    r = r - k * _LN2_LO
    p = np.full_like(x, _TAYLOR[0])
    for c in _TAYLOR[1:]:
        p = p * r + c
    return np.ldexp(p, k.astype(np.int32)).astype(np.float32)


@dataclass(frozen=True)
class SaRun:
    """Moves ``[it_begin, it_begin + iters)`` of chains ``chain_base ..``, the mirror of ``avk::SaRun``;
    the temperature starts at ``temp_start`` (default ``t0``: the run's first segment)."""
    iters: int
    t0: float
    cool: float
    interval: int
    geometric: bool
    max_retry: int
    seed: int
    offset: int = 0
    it_begin: int = 0
    temp_start: float | None = None
    chain_base: int = 0


@dataclass
class SaDomain:
    """What a domain supplies to :func:`sa_chains_twin`; all callables are vectorised over the
    leading (chain) axis of ``sol``."""
    propose: Callable       # (sol, position word x, value word y) -> candidates (a copy)
    valid: Callable         # sol -> bool
    price: Callable         # valid sol -> float32


def sa_cool(temp, it: int, t0, cool, interval: int, geometric: bool) -> np.float32:
    """Step 5: the temperature after move ``it``."""
    if interval > 0 and (it + 1) % interval == 0:
        if geometric:
            return _F(_F(temp) * _F(cool))
        return _F(max(_F(_F(t0) - _F(_F(it + 1) * _F(cool))), _T_MIN))
    return _F(temp)


def sa_temperature(t0, cool, interval: int, geometric: bool, it_begin: int, iters: int, temp_start=None) -> float:
    """The temperature after moves ``[it_begin, it_begin + iters)`` from ``temp_start`` (default ``t0``)."""
    temp = _F(t0 if temp_start is None else temp_start)
    for it in range(it_begin, it_begin + iters):
        temp = sa_cool(temp, it, t0, cool, interval, geometric)
    return float(temp)


def sa_chains_twin(dom: SaDomain, sol, cost, run: SaRun, best=None, best_cost=None):
    """Host twin of optim.hip's ``sa_chain``, vectorised over the chains (the leading axis of ``sol``).
    Returns (best, best_cost, stats, current_sol, current_cost, temperature), as
    :func:`sa_assign_reference`; a run cut into segments through the returned state equals one call."""
    iters, t0, cool, interval, geometric, max_retry, seed, offset, it_begin, temp_start, chain_base = astuple(run)
    sol = np.array(sol)
    P = sol.shape[0]
    c = np.array(cost, dtype=np.float32)
    bc = c.copy() if best_cost is None else np.array(best_cost, dtype=np.float32)
    best = sol.copy() if best is None else np.array(best, dtype=sol.dtype)
    idx = np.arange(P, dtype=np.uint64) + np.uint64(chain_base)
    temp = _F(t0 if temp_start is None else temp_start)
    st = [0, 0, 0]
    R = max_retry + 1
    for it in range(it_begin, it_begin + iters):
        cand = sol.copy()
        todo = np.arange(P)
        for tr in range(R):
            if todo.size == 0:
                break
            x, y, _, _ = philox4x32(seed, offset + it * R + tr, idx[todo])
            attempt = dom.propose(sol[todo], x, y)
            ok = dom.valid(attempt)
            cand[todo[ok]] = attempt[ok]
            todo = todo[~ok]
        moved = np.ones(P, dtype=bool)
        moved[todo] = False
        mv = np.nonzero(moved)[0]
        if mv.size:
            cc = np.asarray(dom.price(cand[mv]), dtype=np.float32)
            cm = c[mv]
            better = cc <= cm
            worse = np.zeros(mv.size, dtype=bool)
            nb = np.nonzero(~better)[0]
            if nb.size:
                x2, _, _, _ = philox4x32(seed ^ _ACCEPT_KEY, offset + it, idx[mv[nb]])
                q = ((cc[nb] - cm[nb]) / np.maximum(temp, _T_MIN)).astype(np.float32)
                worse[nb] = u32_to_unit(x2) < sa_exp(-q)
            acc = better | worse
            st[0] += int(better.sum())
            st[1] += int(worse.sum())
            st[2] += int((~acc).sum())
            a = mv[acc]
            sol[a] = cand[a]
            c[a] = cc[acc]
            imp = a[c[a] < bc[a]]
            best[imp] = sol[imp]
            bc[imp] = c[imp]
        temp = sa_cool(temp, it, t0, cool, interval, geometric)
    return best, bc, {"better": st[0], "worse_accepted": st[1], "rejected": st[2]}, sol, c, temp


def sa_chains_reference(dom: SaDomain, sol, cost, iters: int, t0: float, cool: float, interval: int, geometric: bool,
                        max_retry: int, seed: int, offset: int = 0, it_begin: int = 0, temp_start=None, best=None,
                        best_cost=None, chain_base: int = 0):
    """:func:`sa_chains_twin` with the run spelled out."""
    return sa_chains_twin(dom, sol, cost, SaRun(iters, t0, cool, interval, geometric, max_retry, seed, offset, it_begin,
                                                temp_start, chain_base), best, best_cost)


def sa_chains_init(cards: np.ndarray, valid: Callable, n: int, seed: int, chain_base: int, max_try: int = 40) -> np.ndarray:
    """Start solutions [n, L] int16, host-side per GLOBAL chain: :func:`~avenir_amd.optimize.ga.ga_redraw_init`
    with a pool of one, so the start of chain ``g`` depends on ``(seed, g)`` only and is the same on
    both devices; a start is redrawn while ``valid`` rejects it (the last of ``max_try`` draws stays)."""
    return ga_redraw_init(np.asarray(cards, dtype=np.int64), valid, n, 1, seed, chain_base, max_try)[:, 0]


def sa_chains_launch(kernel: Callable, head: tuple, tail: tuple, sol, cost, run: SaRun, best=None, best_cost=None,
                     device=None):
    """One launch of a native chain kernel, ``kernel(*head, sol, cur_cost, best_sol, best_cost, iters, t0,
    cool, interval, geometric, max_retry, seed, offset, stats, it_begin, temp_start, chain_base, *tail)``,
    on private device copies of the state: numpy (to ``device`` and back) or tensors on the GPU (the
    results stay there).  Returns (best int16, best_cost, stats, sol int16, cost, temperature); this is
    the one place that reads the kernels' ``stats``."""
    resident = isinstance(sol, torch.Tensor)
    if resident and not sol.is_cuda:
        raise ValueError("sa_chains_launch takes numpy state, or tensors that are already on the GPU")

    def own(x, dtype):
        if resident:
            return x.to(dtype=getattr(torch, np.dtype(dtype).name), copy=True).contiguous()
        return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(device)

    s16, cur = own(sol, np.int16), own(cost, np.float32)
    bsol = s16.clone() if best is None else own(best, np.int16)
    bc = cur.clone() if best_cost is None else own(best_cost, np.float32)
    st = torch.zeros(4, dtype=torch.long, device=s16.device)
    ts = float(run.t0 if run.temp_start is None else run.temp_start)
    kernel(*head, s16, cur, bsol, bc, int(run.iters), float(run.t0), float(run.cool), int(run.interval),
           bool(run.geometric), int(run.max_retry), int(run.seed), int(run.offset), st, int(run.it_begin), ts,
           int(run.chain_base), *tail)
    s = st.tolist()
    if run.iters > 0 and s16.shape[0] > 0:
        temp = np.array([s[3]], dtype=np.uint32).view(np.float32)[0]
    else:                                               # nothing was launched: the schedule alone
        temp = _F(sa_temperature(run.t0, run.cool, run.interval, run.geometric, run.it_begin, max(run.iters, 0), ts))
    out = (bsol, bc, s16, cur) if resident else tuple(x.cpu().numpy() for x in (bsol, bc, s16, cur))
    return out[0], out[1], {"better": s[0], "worse_accepted": s[1], "rejected": s[2]}, out[2], out[3], temp


# ---- assignment domains (optim.hip::sa_assign_kernel; the twin is close to it, not bit-equal) ----------
def sa_assign_reference(cost, conflict, swap, sol, cur, iters, t0, cool, interval, geometric, max_retry, seed, offset,
                        it_begin=0, temp_start=None, best=None, best_cost=None, chain_base=0):
    """Host mirror of ``sa_assign_kernel`` (optim.hip), vectorised over chains.  Returns
    (best, best_cost, stats, current_sol, current_cost, temperature)."""
    cost = np.asarray(cost, np.float32)
    L, V = cost.shape
    sol = np.array(sol, dtype=np.int64)
    P = sol.shape[0]
    c = np.array(cur, dtype=np.float32)
    bc = c.copy() if best_cost is None else np.array(best_cost, dtype=np.float32)
    best = sol.copy() if best is None else np.array(best, dtype=np.int64)
    rows = np.arange(P)
    idx = np.arange(P, dtype=np.uint64) + np.uint64(chain_base)
    ar = np.arange(L)
    invL = np.float32(1.0 / L)
    temp = np.float32(t0 if temp_start is None else temp_start)
    st = [0, 0, 0]
    R = max_retry + 1
    for it in range(it_begin, it_begin + iters):
        pending = np.ones(P, bool)
        pos = np.full(P, -1)
        nv = np.zeros(P, np.int64)
        old = np.zeros(P, np.int64)
        j2 = np.full(P, -1)
        for tr in range(R):
            if not pending.any():
                break
            x, y, _, _ = philox4x32(seed, offset + it * R + tr, idx)
            cp = np.minimum((u32_to_unit(x) * np.float32(L)).astype(np.int64), L - 1)
            cv = np.minimum((u32_to_unit(y) * np.float32(V - 1)).astype(np.int64), V - 2)
            ov = sol[rows, cp]
            cv = cv + (cv >= ov)
            if swap:
                holder = (sol == cv[:, None]) & (ar[None, :] != cp[:, None])
                sw = np.where(holder.any(1), holder.argmax(1), -1)
            else:
                sw = np.full(P, -1)
            cand = sol.copy()
            cand[rows, cp] = cv
            hs = sw >= 0
            cand[rows[hs], sw[hs]] = ov[hs]
            if conflict is not None:
                bad = ((cand == cv[:, None]) & (ar[None, :] != cp[:, None]) & conflict[cp]).any(1)
                swr = np.where(hs, sw, 0)
                bad2 = ((cand == ov[:, None]) & (ar[None, :] != swr[:, None]) & conflict[swr]).any(1) & hs
                ok = ~(bad | bad2)
            else:
                ok = np.ones(P, bool)
            take = pending & ok
            sol[take] = cand[take]
            pos[take], nv[take], old[take], j2[take] = cp[take], cv[take], ov[take], sw[take]
            pending &= ~ok
        moved = pos >= 0
        pp = np.where(moved, pos, 0)
        delta = cost[pp, nv] - cost[pp, old]
        jj = np.where(j2 >= 0, j2, 0)
        delta = np.where(j2 >= 0, delta + (cost[jj, old] - cost[jj, nv]), delta).astype(np.float32)
        delta = (delta * invL).astype(np.float32)
        x2, _, _, _ = philox4x32(seed ^ 0x9E3779B97F4A7C15, offset + it, idx)
        with np.errstate(over="ignore"):
            pr = np.exp(-delta / np.maximum(temp, np.float32(1e-12))).astype(np.float32)
        acc = moved & ((delta <= 0) | (u32_to_unit(x2) < pr))
        rej = moved & ~acc
        st[0] += int((acc & (delta <= 0)).sum())
        st[1] += int((acc & (delta > 0)).sum())
        st[2] += int(rej.sum())
        r = rows[rej]
        sol[r, pos[rej]] = old[rej]
        hj = rej & (j2 >= 0)
        sol[rows[hj], j2[hj]] = nv[hj]
        c = np.where(acc, (c + delta).astype(np.float32), c)
        imp = acc & (c < bc)
        best[imp] = sol[imp]
        bc = np.where(imp, c, bc)
        if interval > 0 and (it + 1) % interval == 0:
            temp = np.float32(temp * np.float32(cool)) if geometric else np.float32(max(t0 - (it + 1) * cool, 1e-12))
    return (best, bc.astype(np.float32), {"better": st[0], "worse_accepted": st[1], "rejected": st[2]},
            sol, c.astype(np.float32), temp)


def sa_assign_init(d, n: int, seed: int, chain_base: int, total: int | None = None) -> torch.Tensor:
    """Start solutions [n, L] of global chains ``chain_base ..``: rows of ONE population of ``total`` chains."""
    gen = torch.Generator(device=torch.device(d.device)).manual_seed(int(seed))
    return d.random(chain_base + n if total is None else total, gen)[0][chain_base:chain_base + n]


def sa_assign_advance(d, sol, cost, run: SaRun, device, best=None, best_cost=None):
    """One segment over AssignmentDomain ``d``, as :func:`sa_chains_launch`: the kernel on a GPU, else the twin."""
    if torch.device(device).type == "cuda":
        from .. import _native
        head = (d.cost_table, None if d.conflict is None else d.conflict.to(torch.uint8).contiguous(), bool(d.swap_moves))
        return sa_chains_launch(_native.C().sa_assign, head, (), sol, cost, run, best, best_cost, device)
    return sa_assign_reference(d.cost_table.numpy(), None if d.conflict is None else d.conflict.numpy(), d.swap_moves,
                               sol, cost, *astuple(run)[:10], best, best_cost, run.chain_base)
