"""Island genetic algorithm over an assignment domain as ONE kernel launch (K22,
``csrc/kernels/optim.hip::ga_assign_kernel``) and its bit-exact host twin.

Reference: the Spark GA runs an independent GA per partition (S/optimize/GeneticAlgorithm.scala:70-163);
the Python GeneticAlgorithmOptimizer keeps a pool, crosses random pairs of its mating list and
purges (P/mlextra/optpopu.py:98-187).  Here every island is one workgroup whose pool, costs and
children stay in LDS for all G generations of a launch; its random stream is Philox keyed by the
island's GLOBAL index, so any world size and either device produce the same islands.

:func:`ga_assign_reference` replays the kernel's arithmetic in numpy — the same Philox counters,
the same fp32 cost sums in position order, the same (cost, index) orderings — so GPU output equals
it bit for bit; it is also the CPU path of :class:`~avenir_amd.optimize.search.GeneticAlgorithm`
for assignment domains.

The island frame itself — ranking, ``hist``, the parent and cut draws, the mutation retries, both
replacement policies — is :func:`ga_islands_reference`, the twin of optim.hip's ``ga_island``; the
meeting-schedule and feature-subset twins (:mod:`.ga_meeting`, :mod:`.ga_subset`) run on it too, each
through a :class:`GaDomain` that says what a solution is, when it is valid and what it costs.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable

import numpy as np
import torch

from ..ops.random import philox4x32, u32_to_unit

_MUT_KEY = 0xD1B54A32D192ED03      # the kernel's mutation stream key (seed ^ this)
_INIT_KEY = 0x2545F4914F6CDD1D     # initial pools


_MAX_TRY = 10                      # the kernels' GA_MAX_TRY


def ga_init_population(n_islands: int, P: int, L: int, V: int, seed: int, island_base: int,
                       conflict: np.ndarray | None = None, max_try: int = 40) -> np.ndarray:
    """Initial pools [islands, P, L] int16, position by position as AssignmentDomain.random: the
    value of island gi, member p, position l, attempt a is Philox(seed ^ INIT, (p L + l) 64 + a,
    stream gi), redrawn while it clashes with an earlier conflicting position (up to ``max_try``
    attempts) — per global island, host-side."""
    gis = np.arange(island_base, island_base + n_islands, dtype=np.uint64)
    out = np.zeros((n_islands, P, L), dtype=np.int64)
    for p in range(P):
        for l in range(L):
            todo = np.arange(n_islands)
            for a in range(max_try):
                x, _, _, _ = philox4x32(seed ^ _INIT_KEY, (p * L + l) * 64 + a, gis[todo])
                out[todo, p, l] = np.minimum((u32_to_unit(x) * np.float32(V)).astype(np.int64), V - 1)
                if conflict is None or l == 0:
                    break
                clash = ((out[todo, p, :l] == out[todo, p, l][:, None]) & conflict[l, :l][None, :]).any(1)
                todo = todo[clash]
                if todo.size == 0:
                    break
    return out.astype(np.int16)


def _valid(conf: np.ndarray | None, sol: np.ndarray) -> np.ndarray:
    if conf is None:
        return np.ones(sol.shape[:-1], dtype=bool)
    same = sol[..., :, None] == sol[..., None, :]
    return ~(same & conf).any(axis=(-1, -2))


def ga_price(cost: np.ndarray, conflict: np.ndarray | None, invalid: float, sol: np.ndarray) -> np.ndarray:
    """fp32 sum of cost[l, s_l] in position order times fp32 1/L (the kernel's ``ga_price``), or
    ``invalid`` when two conflicting positions share a value.  sol [..., L] -> [...] float32."""
    L = sol.shape[-1]
    acc = np.zeros(sol.shape[:-1], dtype=np.float32)
    for l in range(L):
        acc = acc + cost[l, sol[..., l]]
    out = acc * (np.float32(1.0) / np.float32(L))
    if conflict is not None:
        same = sol[..., :, None] == sol[..., None, :]
        bad = (same & conflict).any(axis=(-1, -2))
        out = np.where(bad, np.float32(invalid), out).astype(np.float32)
    return out


def _unit_index(u: np.ndarray, n: int) -> np.ndarray:
    """min((int)(u * (float)n), n - 1) in fp32, as the kernel."""
    return np.minimum((u * np.float32(n)).astype(np.int64), n - 1)


def ga_pool_ok(P: int, m: int, r: int, purge_first: bool) -> bool:
    """The island kernels' pool limits (``ga_check_pool`` in optim.hip): one lane per member, per child
    and, when the children join the pool, per candidate."""
    return 2 <= P <= 64 and 1 <= r <= min(P, 32) and 1 <= m <= P and (bool(purge_first) or P + r <= 64)


def ga_assign_lds(P: int, L: int, r: int) -> int:
    """Bytes of LDS of an island's pool view (``avk::ga_assign_lds``): two pools and the children of L
    int16 each, their costs, the two orders and the slot sources, every array rounded up to 16 bytes."""
    a16 = lambda n: (n + 15) & ~15
    return 2 * a16(2 * P * L) + a16(4 * r * L) + 4 * a16(4 * P) + 2 * a16(8 * r)


@dataclass
class GaDomain:
    """What a domain supplies to :func:`ga_islands_reference`.  A pool is [I, P, ...]: L int64 values
    per member, or one uint32 mask; all callables take and return arrays with leading dims [I, r]."""
    encode: Callable        # interface pool int16 [I, P, L] -> working pool
    decode: Callable        # working pool -> int16 [I, P, L]
    ncut: int               # the cut is scale * (1 + unit index into ncut - 1 places), 0 when ncut = 1
    scale: int
    crossover: Callable     # (A, B, cut) -> (head of A + tail of B, head of B + tail of A)
    mutated: Callable       # (c, position word, value word) -> one mutation attempt on a copy of c
    valid: Callable         # c -> bool
    price: Callable         # kids [I, 2r, ...] -> float32 [I, 2r]


def splice(A: np.ndarray, B: np.ndarray, cut: np.ndarray):
    """Single-point crossover of value rows [..., L] at cut [...]."""
    left = np.arange(A.shape[-1]) < cut[..., None]
    return np.where(left, A, B), np.where(left, B, A)


def ga_islands_reference(dom: GaDomain, pop: np.ndarray, pop_cost: np.ndarray, G: int, m: int, r: int,
                         purge_first: bool, mutate: bool, seed: int, island_base: int,
                         gen_base: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Host twin of the island frame of optim.hip (``ga_island``), all islands and all r pairs
    at once: rank by (cost, index), ``hist``, parents and cut of pair k from
    Philox(seed, 256 (gen_base + g) + k, island), each child mutated on Philox(seed ^ MUT, 16 ctr + t,
    island) — words (x, y) for the first child of a pair, (z, w) for the second — until it is valid
    (the last of ``_MAX_TRY`` attempts stays), the best r children replace the worst r members or join
    the pool.  Returns (pop int16, cost float32, hist float32)."""
    pool = dom.encode(pop)
    pc = np.array(pop_cost, dtype=np.float32)
    I, P = pool.shape[:2]
    ar = np.arange(I)
    ii = ar[:, None]
    gir = np.broadcast_to(np.arange(island_base, island_base + I, dtype=np.uint64)[:, None], (I, r))
    hist = np.zeros((I, G), dtype=np.float32)
    for g in range(G):
        ord_ = np.argsort(pc, axis=1, kind="stable")
        hist[:, g] = pc[ar, ord_[:, 0]]
        ctr = np.array([256 * (gen_base + g) + k for k in range(r)], dtype=np.uint64)[None, :]
        x_, y_, z_, _ = philox4x32(seed, np.broadcast_to(ctr, (I, r)), gir)
        a = _unit_index(u32_to_unit(x_), m)
        b = np.zeros((I, r), dtype=np.int64)
        if m > 1:
            b = _unit_index(u32_to_unit(y_), m - 1)
            b = b + (b >= a)
        cut = np.zeros((I, r), dtype=np.int64)
        if dom.ncut > 1:
            cut = dom.scale * (1 + _unit_index(u32_to_unit(z_), dom.ncut - 1))
        pair = list(dom.crossover(pool[ii, ord_[ii, a]], pool[ii, ord_[ii, b]], cut))
        if mutate:
            for h, c in enumerate(pair):
                done = np.zeros((I, r), dtype=bool)
                for t in range(_MAX_TRY):
                    if done.all():
                        break
                    q = philox4x32(seed ^ _MUT_KEY, np.broadcast_to(ctr * np.uint64(16) + np.uint64(t), (I, r)), gir)
                    cand = dom.mutated(c, q[2 * h], q[2 * h + 1])
                    take = ~done & ((t == _MAX_TRY - 1) | dom.valid(cand))
                    c[take] = cand[take]
                    done |= take
        kids = np.stack(pair, axis=2).reshape((I, 2 * r) + pool.shape[2:])     # child 2k, 2k + 1 of pair k
        kc = dom.price(kids)
        kord = np.argsort(kc, axis=1, kind="stable")
        if purge_first:
            nsrc = np.concatenate([ord_[:, : P - r], P + kord[:, :r]], axis=1)
        else:
            src = np.concatenate([np.broadcast_to(np.arange(P), (I, P)), P + kord[:, :r]], axis=1)
            cc = np.concatenate([pc, kc[ii, kord[:, :r]]], axis=1)
            nsrc = np.take_along_axis(src, np.argsort(cc, axis=1, kind="stable")[:, :P], axis=1)
        pool = np.concatenate([pool, kids], axis=1)[ii, nsrc]
        pc = np.concatenate([pc, kc], axis=1)[ii, nsrc]
    return dom.decode(pool), pc, hist


def ga_redraw_init(cards: np.ndarray, valid: Callable, n_islands: int, P: int, seed: int, island_base: int,
                   max_try: int = 40) -> np.ndarray:
    """Initial pools [islands, P, L] int16, host-side per global island: member p of island gi,
    attempt a, position l is min((int)(u card_l), card_l - 1) with u from
    Philox(seed ^ INIT, (p L + l) 64 + a, gi).x; the whole member is redrawn while ``valid`` rejects it
    (up to ``max_try`` <= 64 attempts, the last one stays)."""
    if not 1 <= max_try <= 64:
        raise ValueError("max_try must lie in [1, 64]")
    L = cards.size
    out = np.zeros((n_islands, P, L), dtype=np.int64)
    ti, tp = (x.reshape(-1) for x in np.meshgrid(np.arange(n_islands), np.arange(P), indexing="ij"))
    pos = np.arange(L, dtype=np.uint64)[None, :]
    for a in range(max_try):
        if ti.size == 0:
            break
        off = (tp.astype(np.uint64)[:, None] * np.uint64(L) + pos) * np.uint64(64) + np.uint64(a)
        gis = np.broadcast_to((ti + island_base).astype(np.uint64)[:, None], off.shape)
        x, _, _, _ = philox4x32(seed ^ _INIT_KEY, off, gis)
        draw = np.minimum((u32_to_unit(x) * cards.astype(np.float32)[None, :]).astype(np.int64), cards[None, :] - 1)
        out[ti, tp] = draw
        bad = ~valid(draw)
        ti, tp = ti[bad], tp[bad]
    return out.astype(np.int16)


def ga_islands_launch(kernel: Callable, head: tuple, pop: np.ndarray, pop_cost: np.ndarray, G: int, m: int, r: int,
                      purge_first: bool, mutate: bool, seed: int, island_base: int, gen_base: int, device):
    """One launch of a native island kernel: ``kernel(*head, pop, pop_cost, hist, G, m, r, purge_first,
    mutate, seed, island_base, gen_base)`` on device copies.  Returns numpy (pop, pop_cost, hist)."""
    tp = torch.from_numpy(np.ascontiguousarray(pop, dtype=np.int16)).to(device)
    tc = torch.from_numpy(np.ascontiguousarray(pop_cost, dtype=np.float32)).to(device)
    hist = torch.empty((pop.shape[0], G), dtype=torch.float32, device=device)
    kernel(*head, tp, tc, hist, G, m, r, bool(purge_first), bool(mutate), int(seed), int(island_base), int(gen_base))
    return tp.cpu().numpy(), tc.cpu().numpy(), hist.cpu().numpy()


def _set(c: np.ndarray, pos: np.ndarray, v: np.ndarray) -> None:
    np.put_along_axis(c, pos[..., None], v[..., None], axis=-1)


def ga_assign_domain(cost: np.ndarray, conflict: np.ndarray | None, invalid: float, swap: bool = True) -> GaDomain:
    """What an assignment domain is to the island frames (``ga_assign_kernel``, ``eo_assign_kernel``):
    cost [L, V], conflict [L, L] or None (its upper triangle counts, as in the kernels)."""
    cost = np.ascontiguousarray(cost, dtype=np.float32)
    conf = None
    if conflict is not None:
        conf = np.asarray(conflict, dtype=bool)
        conf = conf & ~np.eye(conf.shape[0], dtype=bool)
        conf = np.triu(conf, 1) | np.triu(conf, 1).T          # the kernel reads the upper triangle
    L, V = cost.shape

    def mutated(c, qp, qv):
        # one position to a different value; with `swap`, the first other position holding that value
        # takes the old one (the domain's swap move)
        pos = _unit_index(u32_to_unit(qp), L)
        old = np.take_along_axis(c, pos[..., None], axis=-1)[..., 0]
        v = _unit_index(u32_to_unit(qv), V - 1)
        v = v + (v >= old)
        cand = c.copy()
        if swap:
            hold = (c == v[..., None]) & (np.arange(L) != pos[..., None])
            _set(cand, np.where(hold.any(-1), hold.argmax(-1), pos), old)
        _set(cand, pos, v)
        return cand

    return GaDomain(encode=lambda p: np.array(p, dtype=np.int64), decode=lambda p: p.astype(np.int16), ncut=L, scale=1,
                    crossover=splice, mutated=mutated, valid=lambda c: _valid(conf, c),
                    price=lambda kids: ga_price(cost, conf, invalid, kids))


def ga_assign_reference(cost: np.ndarray, conflict: np.ndarray | None, invalid: float, pop: np.ndarray,
                        pop_cost: np.ndarray, G: int, m: int, r: int, purge_first: bool, mutate: bool,
                        seed: int, island_base: int, gen_base: int = 0,
                        swap: bool = True) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Host twin of ``ga_assign_kernel`` (all islands at once).  Returns (pop, pop_cost, hist)."""
    dom = ga_assign_domain(cost, conflict, invalid, swap)
    return ga_islands_reference(dom, pop, pop_cost, G, m, r, purge_first, mutate, seed, island_base, gen_base)


def ga_assign_init(domain, n_islands: int, P: int, seed: int, island_base: int) -> tuple[np.ndarray, np.ndarray]:
    """Initial pools of an AssignmentDomain and their costs."""
    conf = None
    if domain.conflict is not None:
        c = domain.conflict.cpu().numpy()
        conf = np.triu(c, 1) | np.triu(c, 1).T
    pop = ga_init_population(n_islands, P, domain.L, domain.V, seed, island_base, conf)
    return pop, ga_price(domain.cost_table.cpu().numpy().astype(np.float32), conf, domain.invalid_cost,
                         pop.astype(np.int64))


def ga_assign_run(domain, pop: np.ndarray, pop_cost: np.ndarray, G: int, m: int, r: int, purge_first: bool,
                  mutate: bool, seed: int, island_base: int, device: torch.device, gen_base: int = 0):
    """Advance the islands G generations (counters from ``gen_base``) on ``device``: the kernel on the
    GPU, the twin on the host.  Returns numpy (pop, pop_cost, hist)."""
    conflict = domain.conflict
    if device.type == "cuda":
        from .. import _native
        cost = domain.cost_table.to(device).float().contiguous()
        cf = None
        if conflict is not None:
            c = conflict.to(device).bool()
            c = c & ~torch.eye(c.shape[0], dtype=torch.bool, device=device)
            cf = (c.triu(1) | c.triu(1).T).to(torch.uint8).contiguous()
        head = (cost, cf, float(domain.invalid_cost), bool(domain.swap_moves))
        return ga_islands_launch(_native.C().ga_assign, head, pop, pop_cost, G, m, r, purge_first, mutate, seed,
                                 island_base, gen_base, device)
    cf = None if conflict is None else conflict.cpu().numpy()
    return ga_assign_reference(domain.cost_table.cpu().numpy(), cf, domain.invalid_cost, pop, pop_cost, G, m, r,
                               purge_first, mutate, seed, island_base, gen_base, bool(domain.swap_moves))
