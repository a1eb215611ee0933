"""Island genetic algorithm over a meeting-schedule domain as ONE kernel launch (K22,
``csrc/kernels/optim.hip::ga_meeting_kernel``) and its bit-exact host twin.

Reference: the GA application of the reference is meeting scheduling (P/app/mesched.py driven by
P/mlextra/optpopu.py:98-187).  The frame is the one of :mod:`~avenir_amd.optimize.ga`: every island
is one workgroup whose pool, costs and children stay in LDS for all G generations of a launch, and
its random stream is Philox keyed by the island's GLOBAL index.  What differs is the domain:

* a solution is (day, hour, minute) index triples of M meetings into integer value tables;
* validity is integer interval arithmetic (participant overlap, blocked hours, ordered pairs);
* the cost is exact in integers up to one short fp32 reduction per solution, people in index order.

:func:`meeting_tables` compiles a :class:`~avenir_amd.optimize.domains.MeetingScheduleDomain` into
the kernel's tables (or ``None`` when it is outside the kernel's limits); :func:`ga_meeting_reference`
replays the kernel in numpy — same Philox counters, same fp32 operations in the same order, same
(cost, index) orderings — so GPU output equals it bit for bit.
"""
from __future__ import annotations

import numpy as np
import torch

from ..ops.random import u32_to_unit
from .ga import (GaDomain, _set, _unit_index, ga_assign_lds, ga_islands_launch, ga_islands_reference, ga_redraw_init,
                 splice)
from .sa import SaDomain, SaRun, sa_chains_init, sa_chains_launch, sa_chains_twin

MAX_M, MAX_Q, MAX_CARD, MAX_LIST = 32, 256, 32, 16      # the kernel's limits
_TIME_LIMIT = 1 << 24                                     # seconds: exact in int32 and in fp32
_F = np.float32


def ga_meeting_lds(P: int, L: int, r: int) -> int:
    """Bytes of LDS per island (``avk::ga_meeting_lds``): the pool view of the frame, the children's
    start / day-bit rows and the staged domain, every array rounded up to 16 bytes."""
    a16 = lambda n: (n + 15) & ~15
    ms = (L // 3) | 1
    return (ga_assign_lds(P, L, r) + 2 * a16(8 * r * ms)
            + a16(4 * (3 * MAX_CARD + 2 * MAX_M + 2 * MAX_Q + 5 * MAX_LIST)))


def _int_values(t) -> np.ndarray | None:
    v = np.asarray(torch.as_tensor(t).detach().cpu().double().numpy(), dtype=np.float64).reshape(-1)
    if not np.isfinite(v).all():
        return None
    r = np.rint(v)
    if not np.array_equal(r, v) or np.abs(r).max(initial=0) >= _TIME_LIMIT:
        return None
    return r.astype(np.int64)


def _masks(rows: np.ndarray) -> np.ndarray:
    """bool [n, M] -> one 32-bit mask per row (bit j = column j), stored as int32."""
    w = np.uint64(1) << np.arange(rows.shape[1], dtype=np.uint64)
    return (rows.astype(np.uint64) * w[None, :]).sum(1).astype(np.uint32).view(np.int32)


def meeting_tables(domain) -> dict | None:
    """The kernel's integer tables and masks of a MeetingScheduleDomain, or ``None`` when the domain
    is outside the kernel's limits (M <= 32, Q <= 256, value tables <= 32, <= 16 blocked entries and
    ordered pairs, all times whole seconds below 2^24) or is no MeetingScheduleDomain."""
    from .domains import MeetingScheduleDomain
    if not isinstance(domain, MeetingScheduleDomain):
        return None
    days, hours, minutes, dur = (_int_values(x) for x in (domain.days, domain.hours, domain.minutes, domain.dur))
    if any(x is None or x.size == 0 for x in (days, hours, minutes, dur)):
        return None
    member = domain.member.cpu().numpy().astype(bool)                     # [Q, M]
    Q, M = member.shape
    if not (1 <= M <= MAX_M and 1 <= Q <= MAX_Q and dur.size == M):
        return None
    if max(days.size, hours.size, minutes.size) > MAX_CARD:
        return None
    if days.min() < 1 or hours.min() < 0 or minutes.min() < 0 or dur.min() < 0:
        return None
    if (days.max() - 1) * 86400 + hours.max() * 3600 + minutes.max() * 60 + dur.max() >= _TIME_LIMIT:
        return None
    share = domain.share.cpu().numpy().astype(bool)
    share = (share | share.T) & ~np.eye(M, dtype=bool)
    blocked = []
    for p, spec in domain.blocked.items():
        b = _int_values(list(spec))
        if b is None or b.size != 3 or not 0 <= int(p) < Q:
            return None
        bs = (b[0] - 1) * 86400 + b[1] * 3600
        be = bs + b[2] * 3600
        if not 0 <= bs <= be < _TIME_LIMIT:
            return None
        blocked.append((int(_masks(member[int(p)][None, :])[0]), int(bs), int(be)))
    if any(len(p) != 2 for p in domain.ordered):
        return None
    ordered = [(int(a), int(b)) for a, b in domain.ordered]
    if len(blocked) > MAX_LIST or len(ordered) > MAX_LIST or any(not (0 <= a < M and 0 <= b < M) for a, b in ordered):
        return None
    role_w = domain.role_w.detach().cpu().numpy().astype(np.float32).reshape(-1)
    if role_w.size != Q:
        return None
    return {
        "M": M, "Q": Q, "L": 3 * M,
        "days": days.astype(np.int32), "hours": hours.astype(np.int32), "minutes": minutes.astype(np.int32),
        "dur": dur.astype(np.int32), "share": _masks(share), "member": _masks(member), "role_w": role_w,
        "blocked": np.array(blocked, dtype=np.int32).reshape(-1, 3),
        "ordered": np.array(ordered, dtype=np.int32).reshape(-1, 2),
        "cards": np.array([days.size, hours.size, minutes.size] * M, dtype=np.int64),
        "share_b": share, "member_b": member, "invalid": float(domain.invalid_cost),
    }


def _times(tb: dict, sol: np.ndarray):
    s = np.asarray(sol, dtype=np.int64)
    st = ((tb["days"].astype(np.int64)[s[..., 0::3]] - 1) * 86400 + tb["hours"].astype(np.int64)[s[..., 1::3]] * 3600
          + tb["minutes"].astype(np.int64)[s[..., 2::3]] * 60)
    return st, st + tb["dur"].astype(np.int64)


def ga_meeting_valid(tables: dict, sol: np.ndarray) -> np.ndarray:
    """Validity of sol [..., 3 M] index triples -> bool [...], integers only (the kernel's ``mt_valid``)."""
    st, en = _times(tables, sol)
    M = tables["M"]
    overlap = (st[..., :, None] < en[..., None, :]) & (st[..., None, :] < en[..., :, None])
    ok = ~(overlap & tables["share_b"]).any(axis=(-1, -2))
    bits = np.arange(M)
    for mask, bs, be in tables["blocked"].tolist():
        mine = ((np.uint32(mask & 0xFFFFFFFF) >> bits.astype(np.uint32)) & np.uint32(1)).astype(bool)
        ok &= ~((st < be) & (bs < en) & mine).any(-1)
    for a, b in tables["ordered"].tolist():
        ok &= en[..., a] <= st[..., b]
    return ok


def ga_meeting_price(tables: dict, sol: np.ndarray) -> np.ndarray:
    """Cost of sol [..., 3 M] -> float32 [...], ``inf`` (the domain's invalid cost) on invalid rows.
    Per person q and day: cnt meetings and booked seconds; over the days with a meeting
    free_q = sum(36000 - booked), nslots_q = sum(cnt + 1), both integers;
    pc = 8 - (free_q / nslots_q) / 3600 and cost = sum(pc w_q) / max(sum(w_q), 1e-12) in fp32,
    accumulated with q ascending, product and sum rounded separately — the kernel's ``mt_cost``."""
    s = np.asarray(sol, dtype=np.int64)
    nd = tables["days"].size
    # float64 products of small integers are exact (and take the BLAS path)
    onehot = (s[..., 0::3, None] == np.arange(nd)).astype(np.float64)                # [..., M, nd]
    mem = tables["member_b"].astype(np.float64)                                      # [Q, M]
    cnt = np.matmul(mem, onehot).astype(np.int64)                                    # [..., Q, nd]
    booked = np.matmul(mem, onehot * tables["dur"].astype(np.float64)[:, None]).astype(np.int64)
    active = cnt > 0
    free = np.where(active, 36000 - booked, 0).sum(-1)                               # [..., Q]
    nslots = np.where(active, cnt + 1, 0).sum(-1)
    num = np.zeros(s.shape[:-1], dtype=np.float32)
    den = np.zeros(s.shape[:-1], dtype=np.float32)
    for q in range(tables["Q"]):
        has = nslots[..., q] > 0
        pc = _F(8.0) - (free[..., q].astype(np.float32) / np.maximum(nslots[..., q], 1).astype(np.float32)) / _F(3600.0)
        w = _F(tables["role_w"][q])
        num = np.where(has, num + pc * w, num).astype(np.float32)
        den = np.where(has, den + w, den).astype(np.float32)
    cost = (num / np.maximum(den, _F(1e-12))).astype(np.float32)
    return np.where(ga_meeting_valid(tables, s), cost, _F(tables["invalid"])).astype(np.float32)


def ga_meeting_init(tables: dict, n_islands: int, P: int, seed: int, island_base: int, max_try: int = 40) -> np.ndarray:
    """Initial pools [islands, P, 3 M] int16: :func:`~avenir_amd.optimize.ga.ga_redraw_init` over the
    value tables' sizes, a member redrawn while it is no valid schedule."""
    return ga_redraw_init(tables["cards"], lambda s: ga_meeting_valid(tables, s), n_islands, P, seed, island_base,
                          max_try)


def _mutated(tables: dict, c: np.ndarray, qp: np.ndarray, qv: np.ndarray) -> np.ndarray:
    """The kernels' move on copies of c [..., 3 M]: position from word qp, a different value of its
    table from word qv; a one-value table keeps its value."""
    cards = tables["cards"]
    pos = _unit_index(u32_to_unit(qp), tables["L"])
    old = np.take_along_axis(c, pos[..., None], axis=-1)[..., 0]
    card = cards[pos]
    v = np.minimum((u32_to_unit(qv) * np.maximum(card - 1, 1).astype(np.float32)).astype(np.int64),
                   np.maximum(card - 2, 0))
    cand = c.copy()
    _set(cand, pos, np.where(card > 1, v + (v >= old), old))
    return cand


def ga_meeting_domain(tables: dict) -> GaDomain:
    """What a meeting-schedule domain is to the island frames (``ga_meeting_kernel``, ``eo_meeting_kernel``);
    the cut falls between two meetings."""
    return GaDomain(encode=lambda p: np.array(p, dtype=np.int64), decode=lambda p: p.astype(np.int16),
                    ncut=tables["M"], scale=3, crossover=splice, mutated=lambda c, qp, qv: _mutated(tables, c, qp, qv),
                    valid=lambda c: ga_meeting_valid(tables, c), price=lambda kids: ga_meeting_price(tables, kids))


def ga_meeting_reference(tables: dict, pop: np.ndarray, pop_cost: np.ndarray, G: int, m: int, r: int,
                         purge_first: bool, mutate: bool, seed: int, island_base: int,
                         gen_base: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Host twin of ``ga_meeting_kernel`` (all islands at once).  Returns (pop int16, cost float32,
    hist float32)."""
    return ga_islands_reference(ga_meeting_domain(tables), pop, pop_cost, G, m, r, purge_first, mutate, seed,
                                island_base, gen_base)


_DEV_KEYS = ("days", "hours", "minutes", "dur", "share", "member", "role_w", "blocked", "ordered")


def _device_tables(tables: dict, device: torch.device) -> list[torch.Tensor]:
    cache = tables.setdefault("_device", {})
    key = str(device)
    if key not in cache:
        cache[key] = [torch.from_numpy(np.ascontiguousarray(tables[k])).to(device) for k in _DEV_KEYS]
    return cache[key]


def ga_meeting_run(domain, pop: np.ndarray, pop_cost: np.ndarray, G: int, m: int, r: int, purge_first: bool,
                   mutate: bool, seed: int, island_base: int, device: torch.device, gen_base: int = 0):
    """Advance the islands G generations (counters from ``gen_base``) on ``device``: the kernel on the
    GPU, the twin on the host.  ``domain`` is a MeetingScheduleDomain or its :func:`meeting_tables`.
    Returns numpy (pop, pop_cost, hist)."""
    tables = domain if isinstance(domain, dict) else meeting_tables(domain)
    if tables is None:
        raise ValueError("the domain is outside the meeting kernel's limits")
    device = torch.device(device)
    if device.type == "cuda":
        from .. import _native
        head = (*_device_tables(tables, device), float(tables["invalid"]))
        return ga_islands_launch(_native.C().ga_meeting, head, pop, pop_cost, G, m, r, purge_first, mutate, seed,
                                 island_base, gen_base, device)
    return ga_meeting_reference(tables, pop, pop_cost, G, m, r, purge_first, mutate, seed, island_base, gen_base)


# ---- simulated-annealing chains (optim.hip::sa_meeting_kernel, frame: optimize/sa.py) ------------------
def sa_meeting_lds(M: int) -> int:
    """Bytes of LDS per 64 chains (``avk::sa_meeting_lds``): the [3 M][64] int16 solutions, the [M][64]
    start seconds and day bits, and the staged domain — 31,680 at M = 32."""
    return 3 * M * 64 * 2 + 2 * M * 64 * 4 + 4 * (3 * MAX_CARD + 2 * MAX_M + 2 * MAX_Q + 5 * MAX_LIST)


def sa_meeting_init(tables: dict, n: int, seed: int, chain_base: int) -> np.ndarray:
    """Start schedules [n, 3 M] int16 of global chains ``chain_base ..`` (:func:`~avenir_amd.optimize.sa.sa_chains_init`)."""
    return sa_chains_init(tables["cards"], lambda s: ga_meeting_valid(tables, s), n, seed, chain_base)


def sa_meeting_advance(tables: dict, sol, cost, run: SaRun, device, best=None, best_cost=None):
    """One segment: ``sa_meeting_kernel`` on a GPU, on the host its twin — the chain frame of
    :mod:`~avenir_amd.optimize.sa` with the island kernel's mutation as the proposal, ``mt_valid`` and
    ``mt_cost``.  Returns (best int16, best_cost, stats, sol int16, cost, temperature)."""
    if torch.device(device).type == "cuda":
        from .. import _native
        return sa_chains_launch(_native.C().sa_meeting, tuple(_device_tables(tables, device)), (), sol, cost, run, best,
                                best_cost, device)
    dom = SaDomain(propose=lambda s, x, y: _mutated(tables, s, x, y), valid=lambda s: ga_meeting_valid(tables, s),
                   price=lambda s: ga_meeting_price(tables, s))
    b, bc, st, s, c, temp = sa_chains_twin(dom, np.array(sol, dtype=np.int64), cost, run,
                                           None if best is None else np.array(best, dtype=np.int64), best_cost)
    return b.astype(np.int16), bc, st, s.astype(np.int16), c, temp


def sa_meeting_reference(tables: dict, sol: np.ndarray, cost: np.ndarray, iters: int, t0: float, cool: float,
                         interval: int, geometric: bool, max_retry: int, seed: int, offset: int = 0, it_begin: int = 0,
                         temp_start=None, best=None, best_cost=None, chain_base: int = 0):
    """Host twin of ``sa_meeting_kernel`` (:func:`sa_meeting_advance` on the host)."""
    return sa_meeting_advance(tables, sol, cost, SaRun(iters, t0, cool, interval, geometric, max_retry, seed, offset,
                                                       it_begin, temp_start, chain_base), "cpu", best, best_cost)


def sa_meeting_run(domain, sol: np.ndarray, cost: np.ndarray, iters: int, t0: float, cool: float, interval: int,
                   geometric: bool, max_retry: int, seed: int, device, offset: int = 0, it_begin: int = 0,
                   temp_start=None, best=None, best_cost=None, chain_base: int = 0):
    """Advance the chains ``iters`` moves (from move ``it_begin``) on ``device``: the kernel on the GPU,
    the twin on the host.  ``domain`` is a MeetingScheduleDomain or its :func:`meeting_tables`.  Returns
    numpy (best int16, best_cost, stats, sol int16, cost, temperature)."""
    tables = domain if isinstance(domain, dict) else meeting_tables(domain)
    if tables is None:
        raise ValueError("the domain is outside the meeting kernel's limits")
    return sa_meeting_advance(tables, sol, cost, SaRun(iters, t0, cool, interval, geometric, max_retry, seed, offset,
                                                       it_begin, temp_start, chain_base), device, best, best_cost)


# ---- evolutionary islands (optim.hip::eo_meeting_kernel, frame: optimize/eo.py) ------------------------
def eo_meeting_advance(tables: dict, pop, cost, run, device, born=None, best=None, best_cost=None):
    """One segment of :class:`~avenir_amd.optimize.eo.EoRun` ``run``: ``eo_meeting_kernel`` on a GPU, on the
    host its twin — the island frame of :mod:`~avenir_amd.optimize.eo` with the island GA's mutation,
    ``mt_valid`` and ``mt_cost``.  Returns (best int16, best_cost, stats, pop int16, cost, born, hist)."""
    from .eo import _numpy_state, eo_islands_launch, eo_islands_reference
    if torch.device(device).type == "cuda":
        from .. import _native
        return eo_islands_launch(_native.C().eo_meeting, tuple(_device_tables(tables, torch.device(device))), pop, cost,
                                 run, born, best, best_cost, torch.device(device))
    return eo_islands_reference(ga_meeting_domain(tables), *_numpy_state(pop, cost), run,
                                *_numpy_state(born, best, best_cost))


def eo_meeting_reference(tables: dict, pop, cost, run, born=None, best=None, best_cost=None, trace: dict | None = None):
    """Host twin of ``eo_meeting_kernel`` (:func:`~avenir_amd.optimize.eo.eo_islands_reference`)."""
    from .eo import eo_islands_reference
    return eo_islands_reference(ga_meeting_domain(tables), pop, cost, run, born, best, best_cost, trace)
