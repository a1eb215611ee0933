"""Island genetic algorithm over feature subsets scored by naive Bayes as ONE kernel launch (K22,
``csrc/kernels/optim.hip::ga_subset_kernel``), the scoring on its own
(``subset_errors_kernel``) and their bit-exact host twins.

Reference: feature selection is the second population-search application of the reference
(P/app/fesel.py driven by P/mlextra/optpopu.py:98-187).  The frame is the one of
:mod:`~avenir_amd.optimize.ga_meeting`: every island is one workgroup whose pool, costs and children
stay in LDS for all G generations of a launch, and its random stream is Philox keyed by the island's
GLOBAL index.  What differs is the domain:

* a solution is a 32-bit mask over F <= 32 features (int16 0 / 1 rows at the interface), valid when
  ``min_size <= popcount <= max_size``; mutation flips one bit;
* the cost is the naive-Bayes error of the subset: with per-row, per-feature, per-class
  log-likelihoods ``LL [N, F, C]`` the score of row n and class c is ``log_prior[c]`` plus
  ``LL[n, f, c]`` over the included features, f ascending, one fp32 add each; the prediction is the
  first class with the largest score and the cost is ``(float)errors / (float)N``.  The error count
  is an integer, so it depends on no tile, grid or workgroup size.

:func:`subset_tables` compiles a :class:`~avenir_amd.optimize.domains.FeatureSubsetDomain` with the
built-in evaluator into the kernels' tables (or ``None``); :func:`subset_errors_reference` and
:func:`ga_subset_reference` replay the kernels in numpy — same Philox counters, same fp32 adds in the
same order, same (cost, index) orderings — so GPU output equals them bit for bit.
"""
from __future__ import annotations

import numpy as np
import torch

from ..ops.random import u32_to_unit
from .ga import GaDomain, _unit_index, ga_islands_launch, ga_islands_reference, ga_redraw_init
from .sa import SaDomain, SaRun, sa_chains_init, sa_chains_launch, sa_chains_twin

MAX_F, MAX_C, MAX_N = 32, 16, 1 << 24                   # the kernels' limits: F <= 32, C <= 16, N < 2^24
# GeneticAlgorithm takes the island engine up to this many rows (search._island_engine): the largest
# size at which one island still beat the generic path (profiles/ga_subset_cap_sweep.jsonl)
ROW_CAP = 1 << 15
# SimulatedAnnealing takes the chain engine by default up to this many rows (search._chain_engine):
# one chain of 300 moves took 145 ms against 170 ms at 2^17 rows and 288 ms against 171 ms at 2^18
# (profiles/sa_subset_cap_sweep.jsonl); 1,024 chains still win 5.6 x at 2^16 rows
SA_ROW_CAP = 1 << 17
# EvolutionaryOptimizer takes the island engine by default up to this many rows (search._island_engine):
# one island is one workgroup that streams every row once per iteration, and one island of 300
# iterations took 147 ms against 326 ms at 2^17 rows, 288 ms against 307 ms at 2^18 (inside the spread
# of the runs: no win) and 578 ms against 288 ms at 2^19 (profiles/eo_subset_cap_sweep.jsonl); 1,024
# islands still win 6.5 x at 2^16 rows
EO_ROW_CAP = 1 << 17
_F = np.float32


def ga_subset_lds(N: int, F: int, C: int) -> int:
    """Bytes of dynamic LDS per island (``avk::ga_subset_lds``): the row tile, a power of two of at
    most 256 (N <= 2048) or 1,024 rows of odd stride ``F C | 1`` within 48 KiB, at least 16 rows."""
    tr = 1024 if N > 2048 else 256
    stride = (F * C) | 1
    while tr > 16 and tr * stride * 4 > 48 * 1024:
        tr >>= 1
    return tr * stride * 4


def _key(domain) -> tuple:
    t = (domain.loglik, domain.log_prior, domain.labels)
    return tuple((id(x), x._version) for x in t) + (domain.min_size, domain.max_size)


def subset_tables(domain) -> dict | None:
    """The kernels' tables of a FeatureSubsetDomain with the built-in naive-Bayes evaluator, or
    ``None``: a ``cost_fn``, no ``loglik``, tied ``groups``, a shape outside the limits (1 <= F <= 32,
    2 <= C <= 16, 1 <= N < 2^24, labels in int32) or a non-finite value in ``loglik`` / ``log_prior``
    (``-inf`` too).  The tables are kept on the domain while its tensors stay unchanged."""
    from .domains import FeatureSubsetDomain
    if not isinstance(domain, FeatureSubsetDomain) or domain.cost_fn is not None or domain.groups:
        return None
    ll, lp, lab = domain.loglik, domain.log_prior, domain.labels
    if ll is None or lp is None or lab is None or ll.dim() != 3:
        return None
    key = _key(domain)
    hit = domain.__dict__.get("_subset_tables")
    if hit is not None and hit[0] == key:
        return hit[1]
    N, F, C = ll.shape
    tables = None
    if (1 <= F <= MAX_F and F == domain.F and 2 <= C <= MAX_C and 1 <= N < MAX_N and lp.numel() == C
            and lab.numel() == N and 0 <= domain.min_size <= min(domain.max_size, MAX_F)
            and bool(torch.isfinite(ll).all()) and bool(torch.isfinite(lp).all())
            and int(lab.min()) >= -(1 << 31) and int(lab.max()) < (1 << 31)):
        dll = ll.detach().float().contiguous()
        dlp = lp.detach().float().reshape(-1).contiguous()
        dlab = lab.detach().reshape(-1).to(torch.int32).contiguous()
        tables = {
            "N": int(N), "F": int(F), "C": int(C),
            "LL": np.ascontiguousarray(dll.cpu().numpy()), "log_prior": np.ascontiguousarray(dlp.cpu().numpy()),
            "labels": np.ascontiguousarray(dlab.cpu().numpy()),
            "min_size": int(domain.min_size), "max_size": min(int(domain.max_size), MAX_F),
            "invalid": float(domain.invalid_cost), "_device": {},
        }
        if ll.device.type == "cuda":                       # the domain's own tensors serve its device
            tables["_device"][_dev_key(ll.device)] = [dll, dlp, dlab]
    domain.__dict__["_subset_tables"] = (key, tables)
    return tables


def _dev_key(device: torch.device) -> str:
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        return f"cuda:{torch.cuda.current_device()}"
    return str(device)


def _device_tables(tables: dict, device: torch.device) -> list[torch.Tensor]:
    cache = tables.setdefault("_device", {})
    key = _dev_key(device)
    if key not in cache:
        cache[key] = [torch.from_numpy(tables[k]).to(device) for k in ("LL", "log_prior", "labels")]
    return cache[key]


def pack_masks(sol) -> np.ndarray:
    """0 / 1 rows [..., F] -> uint32 masks [...] (bit f = column f)."""
    s = np.asarray(sol)
    w = np.uint64(1) << np.arange(s.shape[-1], dtype=np.uint64)
    return ((s != 0).astype(np.uint64) * w).sum(-1).astype(np.uint32)


def unpack_masks(masks, F: int) -> np.ndarray:
    """uint32 masks [...] -> int16 0 / 1 rows [..., F]."""
    mk = np.asarray(masks, dtype=np.uint32)
    return ((mk[..., None] >> np.arange(F, dtype=np.uint32)) & np.uint32(1)).astype(np.int16)


def _as_masks(masks) -> np.ndarray:
    if isinstance(masks, torch.Tensor):
        masks = masks.detach().cpu().numpy()
    mk = np.asarray(masks)
    if mk.dtype == np.int32:
        return mk.view(np.uint32).reshape(-1)
    if mk.size and (mk.min() < 0 or mk.max() >= (1 << 32)):
        raise ValueError("masks must fit 32 bits")
    return mk.astype(np.uint32).reshape(-1)


def _field(F: int) -> np.uint32:
    return np.uint32(0xFFFFFFFF if F == 32 else (1 << F) - 1)


def subset_errors_reference(tables: dict, masks) -> np.ndarray:
    """Host twin of ``subset_errors_kernel``: int64 [B] rows mis-predicted under each 32-bit mask.
    Scores [N, C] start at the prior and, for f ascending, become
    ``np.where(bit_f, (s + LL[:, f, :]).astype(float32), s)`` — for one mask at a time that is an
    fp32 add for every set bit and nothing otherwise; the first maximum over the classes predicts.
    Equal masks are scored once."""
    mk = _as_masks(masks) & _field(tables["F"])
    lp, lab = tables["log_prior"], tables["labels"]
    N, F, C = tables["LL"].shape
    if "_LLT" not in tables:                                 # [F, N, C]: one contiguous slab per feature
        tables["_LLT"] = np.ascontiguousarray(tables["LL"].transpose(1, 0, 2))
    llt = tables["_LLT"]
    uniq, inv = np.unique(mk, return_inverse=True)
    err = np.zeros(uniq.size, dtype=np.int64)
    for i, u in enumerate(uniq.tolist()):
        s = np.broadcast_to(lp[None, :], (N, C)).astype(np.float32)
        for f in range(F):
            if (u >> f) & 1:
                np.add(s, llt[f], out=s)
        err[i] = np.count_nonzero(s.argmax(1) != lab)
    return err[inv.reshape(-1)]


def subset_errors(tables: dict, masks, device="cpu") -> np.ndarray:
    """Error counts int64 [B] of 32-bit masks: ``subset_errors_kernel`` on a GPU, the twin on the host."""
    device = torch.device(device)
    if device.type != "cuda":
        return subset_errors_reference(tables, masks)
    mk = torch.from_numpy(_as_masks(masks).view(np.int32).copy()).to(device)
    return subset_errors_device(tables, mk).cpu().numpy().astype(np.int64)


def subset_errors_device(tables: dict, masks: torch.Tensor) -> torch.Tensor:
    """``subset_errors_kernel`` on int32 masks [B] resident on a GPU -> int32 [B] on that GPU."""
    from .. import _native
    return _native.C().subset_errors(*_device_tables(tables, masks.device), masks.contiguous())


def ga_subset_valid(tables: dict, masks) -> np.ndarray:
    """min_size <= popcount <= max_size of uint32 masks [...] -> bool [...]."""
    mk = np.asarray(masks, dtype=np.uint32)
    n = unpack_masks(mk, 32).sum(-1)
    return (n >= tables["min_size"]) & (n <= tables["max_size"])


def ga_subset_price(tables: dict, masks, device="cpu") -> np.ndarray:
    """Cost float32 [...] of uint32 masks [...]: ``(float)errors / (float)N``, the domain's invalid
    cost for an invalid mask (which is not scored)."""
    mk = np.asarray(masks, dtype=np.uint32)
    ok = ga_subset_valid(tables, mk)
    cost = np.full(mk.shape, _F(tables["invalid"]), dtype=np.float32)
    if ok.any():
        err = subset_errors(tables, mk[ok], device)
        cost[ok] = err.astype(np.float32) / _F(tables["N"])
    return cost


def ga_subset_init(tables: dict, n_islands: int, P: int, seed: int, island_base: int, max_try: int = 40) -> np.ndarray:
    """Initial pools [islands, P, F] int16 of 0 / 1: :func:`~avenir_amd.optimize.ga.ga_redraw_init`
    with two values per position, a member redrawn while its size is out of range."""
    return ga_redraw_init(np.full(tables["F"], 2, dtype=np.int64), lambda s: ga_subset_valid(tables, pack_masks(s)),
                          n_islands, P, seed, island_base, max_try)


def ga_subset_domain(tables: dict, price=None) -> GaDomain:
    """What a feature-subset domain is to the island frames (``ga_subset_kernel``, ``eo_subset_kernel``): a
    solution is one uint32 mask, a mutation flips one bit (the value draw is unused)."""
    F = tables["F"]

    def crossover(A, B, cut):
        low = ((np.uint64(1) << cut.astype(np.uint64)) - np.uint64(1)).astype(np.uint32)      # cut <= 31
        return (A & low) | (B & ~low), (B & low) | (A & ~low)

    def mutated(c, qp, qv):
        return c ^ (np.uint32(1) << _unit_index(u32_to_unit(qp), F).astype(np.uint32))

    return GaDomain(encode=pack_masks, decode=lambda mk: unpack_masks(mk, F), ncut=F, scale=1, crossover=crossover,
                    mutated=mutated, valid=lambda c: ga_subset_valid(tables, c),
                    price=price or (lambda kids: ga_subset_price(tables, kids)))


def ga_subset_reference(tables: dict, pop: np.ndarray, pop_cost: np.ndarray, G: int, m: int, r: int,
                        purge_first: bool, mutate: bool, seed: int, island_base: int,
                        gen_base: int = 0) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Host twin of ``ga_subset_kernel`` (all islands at once).  Returns (pop int16, cost float32,
    hist float32)."""
    return ga_islands_reference(ga_subset_domain(tables), pop, pop_cost, G, m, r, purge_first, mutate, seed,
                                island_base, gen_base)


def ga_subset_run(domain, pop: np.ndarray, pop_cost: np.ndarray, G: int, m: int, r: int, purge_first: bool,
                  mutate: bool, seed: int, island_base: int, device: torch.device, gen_base: int = 0):
    """Advance the islands G generations (counters from ``gen_base``) on ``device``: the kernel on the
    GPU, the twin on the host.  ``domain`` is a FeatureSubsetDomain or its :func:`subset_tables`.
    Returns numpy (pop int16, pop_cost float32, hist float32)."""
    tables = domain if isinstance(domain, dict) else subset_tables(domain)
    if tables is None:
        raise ValueError("the domain is outside the subset kernel's limits")
    pop = np.ascontiguousarray(pop, dtype=np.int16)
    if pop.ndim != 3 or pop.shape[2] != tables["F"]:
        raise ValueError("pop must be [islands, P, F]")
    if pop.size and (pop.min() < 0 or pop.max() > 1):
        raise ValueError("pool values must be 0 or 1")
    device = torch.device(device)
    if device.type == "cuda":
        from .. import _native
        head = (*_device_tables(tables, device), tables["min_size"], tables["max_size"], float(tables["invalid"]))
        return ga_islands_launch(_native.C().ga_subset, head, pop, pop_cost, G, m, r, purge_first, mutate, seed,
                                 island_base, gen_base, device)
    return ga_subset_reference(tables, pop, pop_cost, G, m, r, purge_first, mutate, seed, island_base, gen_base)


# ---- simulated-annealing chains (optim.hip::sa_subset_kernel, frame: optimize/sa.py) -------------------
def sa_subset_init(tables: dict, n: int, seed: int, chain_base: int) -> np.ndarray:
    """Start subsets [n, F] int16 of 0 / 1 of global chains ``chain_base ..``
    (:func:`~avenir_amd.optimize.sa.sa_chains_init`)."""
    return sa_chains_init(np.full(tables["F"], 2, dtype=np.int64), lambda s: ga_subset_valid(tables, pack_masks(s)),
                          n, seed, chain_base)


def sa_subset_advance(tables: dict, sol, cost, run: SaRun, device, best=None, best_cost=None, waves_per_chain: int = 0):
    """One segment: ``sa_subset_kernel`` on a GPU (``waves_per_chain`` = 0 lets the launcher choose; no
    result depends on it), on the host its twin — the chain frame of :mod:`~avenir_amd.optimize.sa`
    over 32-bit masks: a move flips one bit (the value word is unused), a mask is valid inside the
    size range and costs ``(float)errors / (float)N``; a mask is scored once per call.  Returns (best
    int16 0 / 1 rows, best_cost, stats, sol int16, cost, temperature)."""
    if torch.device(device).type == "cuda":
        from .. import _native
        head = (*_device_tables(tables, device), tables["min_size"], tables["max_size"])
        return sa_chains_launch(_native.C().sa_subset, head, (int(waves_per_chain),), sol, cost, run, best, best_cost,
                                device)
    F, N = tables["F"], _F(tables["N"])
    seen: dict = {}

    def price(mk):
        new = np.array(sorted(set(mk.tolist()) - seen.keys()), dtype=np.uint32)
        if new.size:
            seen.update(zip(new.tolist(), subset_errors_reference(tables, new).tolist()))
        return np.array([seen[m] for m in mk.tolist()], dtype=np.float32) / N

    dom = SaDomain(propose=lambda s, x, y: s ^ (np.uint32(1) << _unit_index(u32_to_unit(x), F).astype(np.uint32)),
                   valid=lambda s: ga_subset_valid(tables, s), price=price)
    b, bc, st, s, c, temp = sa_chains_twin(dom, pack_masks(sol), cost, run, None if best is None else pack_masks(best),
                                           best_cost)
    return unpack_masks(b, F), bc, st, unpack_masks(s, F), c, temp


def sa_subset_reference(tables: dict, sol: np.ndarray, cost: np.ndarray, iters: int, t0: float, cool: float,
                        interval: int, geometric: bool, max_retry: int, seed: int, offset: int = 0, it_begin: int = 0,
                        temp_start=None, best=None, best_cost=None, chain_base: int = 0):
    """Host twin of ``sa_subset_kernel`` (:func:`sa_subset_advance` on the host)."""
    return sa_subset_advance(tables, sol, cost, SaRun(iters, t0, cool, interval, geometric, max_retry, seed, offset,
                                                      it_begin, temp_start, chain_base), "cpu", best, best_cost)


def sa_subset_run(domain, sol: np.ndarray, cost: np.ndarray, iters: int, t0: float, cool: float, interval: int,
                  geometric: bool, max_retry: int, seed: int, device, offset: int = 0, it_begin: int = 0,
                  temp_start=None, best=None, best_cost=None, chain_base: int = 0, waves_per_chain: int = 0):
    """Advance the chains ``iters`` moves (from move ``it_begin``) on ``device``: the kernel on the GPU,
    the twin on the host.  ``domain`` is a FeatureSubsetDomain or its :func:`subset_tables`.  Returns
    numpy (best int16, best_cost, stats, sol int16, cost, temperature)."""
    tables = domain if isinstance(domain, dict) else subset_tables(domain)
    if tables is None:
        raise ValueError("the domain is outside the subset kernel's limits")
    sol = np.ascontiguousarray(sol, dtype=np.int16)
    if sol.ndim != 2 or sol.shape[1] != tables["F"]:
        raise ValueError("sol must be [chains, F]")
    run = SaRun(iters, t0, cool, interval, geometric, max_retry, seed, offset, it_begin, temp_start, chain_base)
    return sa_subset_advance(tables, sol, cost, run, device, best, best_cost, waves_per_chain)


# ---- evolutionary islands (optim.hip::eo_subset_kernel, frame: optimize/eo.py) -------------------------
def eo_subset_advance(tables: dict, pop, cost, run, device, born=None, best=None, best_cost=None,
                      waves_per_island: int = 0):
    """One segment of :class:`~avenir_amd.optimize.eo.EoRun` ``run``: ``eo_subset_kernel`` on a GPU
    (``waves_per_island`` = 0 lets the launcher choose; no result depends on it), on the host its twin —
    the island frame of :mod:`~avenir_amd.optimize.eo` over 32-bit masks: a mutation flips one bit, a
    mask is valid inside the size range and costs ``(float)errors / (float)N``; the twin scores a mask
    once per call.  Returns (best int16 0 / 1 rows, best_cost, stats, pop int16, cost, born, hist)."""
    from .eo import _numpy_state, eo_islands_launch, eo_islands_reference
    if torch.device(device).type == "cuda":
        from .. import _native
        device = torch.device(device)
        kernel = lambda *a: _native.C().eo_subset(*a, int(waves_per_island))
        head = (*_device_tables(tables, device), tables["min_size"], tables["max_size"])
        return eo_islands_launch(kernel, head, pop, cost, run, born, best, best_cost, device)
    pop, cost, born, best, best_cost = _numpy_state(pop, cost, born, best, best_cost)
    for s in (pop, best):
        if s is not None and np.size(s) and (np.min(s) < 0 or np.max(s) > 1):
            raise ValueError("eo_subset: masks must be 0 or 1")
    N = _F(tables["N"])
    seen: dict = {}

    def price(mk):                                           # only valid masks are priced
        flat = np.asarray(mk, dtype=np.uint32).reshape(-1)
        new = np.array(sorted(set(flat.tolist()) - seen.keys()), dtype=np.uint32)
        if new.size:
            seen.update(zip(new.tolist(), subset_errors_reference(tables, new).tolist()))
        return (np.array([seen[m] for m in flat.tolist()], dtype=np.float32) / N).reshape(np.shape(mk))

    return eo_islands_reference(ga_subset_domain(tables, price), pop, cost, run, born, best, best_cost)


def eo_subset_reference(tables: dict, pop, cost, run, born=None, best=None, best_cost=None, trace: dict | None = None):
    """Host twin of ``eo_subset_kernel`` (:func:`~avenir_amd.optimize.eo.eo_islands_reference`)."""
    from .eo import eo_islands_reference
    return eo_islands_reference(ga_subset_domain(tables), pop, cost, run, born, best, best_cost, trace)
