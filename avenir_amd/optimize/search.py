"""Batched stochastic optimisers (K22): simulated annealing, genetic algorithm (island model),
evolutionary strategy, random multi-start search with local search, tabu search, Bayesian
optimisation, and hyper-parameter search.

Reference behaviour:
* Spark SA — one chain per partition, Metropolis acceptance, geometric/linear cooling every
  ``temp.update.interval`` moves, accumulators, optional local search of each chain's best
  (S/optimize/SimulatedAnnealing.scala:111-234; config R/opt.conf).
* Spark GA — island model, each partition an independent GA (S/optimize/GeneticAlgorithm.scala:70-163).
* Spark random search — random multi-start then ``focussed`` (neighbours of the best) or
  ``trajectory`` local search (S/optimize/RandomSearch.scala:105-250).
* Python optimisers — ``EvolutionaryOptimizer`` / ``GeneticAlgorithmOptimizer`` (P/mlextra/optpopu.py:32-187,
  pool / mating / replacement / purge-by-cost-and-age), ``SimulatedAnnealingOptimizer`` and
  ``BayesianOptimizer`` (P/mlextra/optsolo.py:34-182); parameter search (P/supv/pasearch.py:17-242);
  ``TabuSearchDomain`` tenure purge (J/optimize/TabuSearchDomain.java:54-66).

MI355X design: the population / the set of chains / the set of islands is the batch axis of
device tensors.  Simulated annealing over an :class:`AssignmentDomain` runs entirely inside one
K22 kernel launch (one chain per lane, solution tile in LDS); over meeting-schedule and
feature-subset domains it runs in the chain kernels of optimize/sa.py (``sa_meeting_kernel``: one
chain per lane; ``sa_subset_kernel``: 1 to 16 waves per chain over a shared row tile), whose numpy
twins they equal bit for bit, the Metropolis decision included.  So does the island genetic
algorithm (optimize/ga.py: one workgroup per island, pool / costs / children in LDS, all
generations of a migration interval per launch; its numpy twin is the CPU path, bit-equal).
Tabu search over an :class:`AssignmentDomain` on a GPU is one launch of ``tabu_assign_kernel``
(optimize/tabu.py: one chain per wave; tabu table, blocked counts, solution in LDS; the full
L x V neighbourhood scored and reduced inside the wave every iteration), bit-equal to its numpy
twin; the torch path (three [P, L, V] tensors, a validity GEMM and five host reads per iteration)
stays the CPU default.
The evolutionary optimiser over assignment, meeting-schedule and feature-subset domains on a GPU is
one launch of ``eo_assign_kernel`` / ``eo_meeting_kernel`` (optimize/eo.py: one island per lane; pool,
costs, age ranks and clone in lane-private LDS columns; tournament, mutation with take-back, pricing
and purge inside the lane every iteration) or ``eo_subset_kernel`` (1 to 16 waves per island over a
shared row tile, one pool member per lane in registers), bit-equal to its numpy twin, with global
islands and explicit resumable state; its torch path (about 15 launches and a host read per
iteration) stays the CPU default and serves callback and grouped domains.
Other domains take batched tensor ops per generation; the GA over them runs one generation per
ISLAND (each island draws from its own generator, keyed by global island index, so that results do
not depend on the world size): ~12 small launches per island per generation.  Measured on one
MI355X (profiles/r6_ga_islands.jsonl): 8 / 64 / 512 islands x 50 generations at 3.9 k / 20.5 k /
110 k island-generations/s end to end with the kernel, 316 / 310 with the per-island path.
Chains and islands are indexed GLOBALLY (their random streams
are keyed by global index, not by rank): rank r runs its block of them, the W-rank run equals one
process running all of them, the global best is one tiny all-gather, and checkpoints re-deal the
chains / islands over any world size on resume.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from functools import partial
from typing import Callable, Sequence

import numpy as np
import torch

from ..parallel.comm import Comm, get_comm
from ..utils.resilience import IterationLoop, RecoveryConfig
from .domain import AssignmentDomain, SearchDomain
from .sa import SaRun, sa_assign_advance, sa_assign_init, sa_assign_reference  # noqa: F401 (the twin is re-exported)


@dataclass
class OptResult:
    best: torch.Tensor                 # [L] best solution (value indices)
    best_cost: float
    costs: torch.Tensor                # [n] best cost per chain / island (local rank)
    solutions: torch.Tensor            # [n, L]
    history: list = field(default_factory=list)
    stats: dict = field(default_factory=dict)


def _gen(device, seed: int) -> torch.Generator:
    return torch.Generator(device=torch.device(device)).manual_seed(int(seed))


def _global_best(comm: Comm, cost: torch.Tensor, sol: torch.Tensor) -> tuple[torch.Tensor, float]:
    if cost.numel() == 0:                  # a rank left without chains / islands after a re-deal
        c, s = torch.full((1,), math.inf, device=cost.device), torch.zeros(sol.shape[-1], dtype=torch.long,
                                                                            device=sol.device)
    else:
        i = int(torch.argmin(cost))
        c, s = cost[i:i + 1].float(), sol[i].long()
    if comm.is_distributed:
        dev = comm.device if comm.backend == "nccl" else torch.device("cpu")
        cs = comm.all_gather(c.to(dev)).view(-1)
        ss = comm.all_gather(s.to(dev))
        j = int(torch.argmin(cs))
        return ss[j].to(sol.device), float(cs[j])
    return s, float(c)


# ================================================================================================
# simulated annealing
# ================================================================================================
class _Chains:
    """A chain engine: one of the chain kernels of optim.hip on a GPU, its host twin on the CPU.
    ``names`` are the (GPU, CPU) engine names of ``OptResult.stats`` (None: no entry);
    ``init(n, seed, chain_base)`` draws start solutions, ``price(sol)`` is their cost (numpy or tensors)
    and ``run(sol, cost, SaRun, device, best, best_cost)`` advances them (``ga_meeting.sa_meeting_advance``)."""

    def __init__(self, names, init, price, run):
        self.names, self.init, self.price, self.run = names, init, price, run

    def start(self, device, n: int, seed: int, chain_base: int) -> torch.Tensor:
        return torch.as_tensor(self.init(n, seed, chain_base)).long().to(device)

    def cost(self, device, sol: torch.Tensor) -> torch.Tensor:
        return torch.as_tensor(self.price(sol), dtype=torch.float32).to(device)

    def advance(self, device, sol, cost, run: SaRun, best=None, best_cost=None):
        """Tensors on ``device`` in and out; a kernel takes them where they are, a host twin as numpy."""
        state = [sol, cost, best, best_cost]
        if device.type != "cuda":
            state = [None if t is None else t.detach().numpy() for t in state]
        b, bc, stats, s, c, temp = self.run(*state[:2], run, device, *state[2:])
        return (torch.as_tensor(b).long(), torch.as_tensor(bc), stats, torch.as_tensor(s).long(), torch.as_tensor(c),
                float(temp))


class SimulatedAnnealing:
    """Batched SA chains.  The one-launch K22 kernel (``sa_assign_kernel``) takes assignment domains
    with single-position moves (``max.step.size`` = 1) and L <= 512 positions (the [L][64]
    solution tile of a wave lives in LDS).  Meeting-schedule and feature-subset domains inside the
    limits of their kernels take ``sa_meeting_kernel`` / ``sa_subset_kernel`` (one launch per run or
    checkpoint segment, bit-equal host twins; :meth:`_chain_engine`).  Multi-position steps, larger
    L and other domains run the batched generic path: every chain of the rank advances together,
    one set of tensor ops per move (documented limit; the reference's task-schedule configurations
    all use step 1 and tens of positions)."""

    def __init__(self, domain: SearchDomain, n_chains: int = 8, iters: int = 300, t0: float = 30.0,
                 cooling: float = 0.99, geometric: bool = True, interval: int = 2, step: int = 1,
                 max_retry: int = 3, seed: int = 0, locally_optimize: bool = False, local_iters: int = 50,
                 comm: Comm | None = None, use_kernel: bool | None = None,
                 recovery: RecoveryConfig | None = None, segment: int | None = None):
        self.domain = domain
        self.recovery = recovery        # checkpoint / resume (utils/resilience)
        self.segment = segment          # moves per checkpointed segment (default iters / 10)
        self.n_chains, self.iters, self.t0, self.cooling = n_chains, iters, t0, cooling
        self.geometric, self.interval, self.step, self.max_retry = geometric, interval, step, max_retry
        self.seed, self.locally_optimize, self.local_iters = seed, locally_optimize, local_iters
        self.comm = comm
        self.use_kernel = use_kernel

    @classmethod
    def from_config(cls, domain, cfg, **kw) -> "SimulatedAnnealing":
        """HOCON block of R/opt.conf (``simulatedAnnealing``)."""
        return cls(domain, n_chains=cfg.get_int("num.optimizers"), iters=cfg.get_int("max.num.iterations"),
                   t0=cfg.get_float("initial.temp", 30.0), cooling=cfg.get_float("cooling.rate.value", 0.99),
                   geometric=cfg.get_bool("cooling.rate.geometric", True),
                   interval=cfg.get_int("temp.update.interval", 2), step=cfg.get_int("max.step.size", 1),
                   locally_optimize=cfg.get_bool("locally.optimize", False),
                   local_iters=cfg.get_int("max.num.local iterations", cfg.get_int("max.num.local.iterations", 50)),
                   **kw)

    def run(self, init: torch.Tensor | None = None) -> OptResult:
        comm = self.comm or get_comm()
        d = self.domain
        engine = self._chain_engine(comm.world)
        chain_base = None
        if engine is not None:
            best, bc, stats, chain_base = self._run_kernel(comm, init, engine)
        else:
            seed = self.seed + 1_000_003 * comm.rank
            gen = _gen(d.device, seed)
            sol = d.random(self.n_chains, gen)[0] if init is None else init.to(d.device).long().clone()
            # generic path: one torch generator per rank drives every chain of the rank -> sharded
            # state, resumable at the world size that wrote it
            with IterationLoop("simulatedAnnealing.generic", self.recovery, comm, sharded=True,
                               device=d.device) as lp:
                best, bc, stats = self._generic(sol, d.evaluate(sol), gen, lp)
        if self.locally_optimize:
            if chain_base is None:      # generic path: the rank's generator (as its chains)
                best, bc = local_focussed(d, best, bc, self.local_iters, gen)
            else:                       # kernel path: one generator per GLOBAL chain, so the result
                outs = [local_focussed(d, best[p:p + 1], bc[p:p + 1], self.local_iters,  # does not depend on W
                                       _gen(d.device, self.seed + 1_000_003 + chain_base + p))
                        for p in range(best.shape[0])]
                if outs:
                    best = torch.cat([o[0] for o in outs])
                    bc = torch.cat([o[1] for o in outs])
        b, c = _global_best(comm, bc, best)
        return OptResult(b, c, bc, best, stats=stats)

    def _chain_engine(self, world: int = 1):
        """The one-launch chain kernel that applies to the domain, or None (the generic torch path):
        single-position moves and no tied groups.  An AssignmentDomain of L <= 512 positions takes
        ``sa_assign_kernel`` or, on the CPU, its twin unless ``use_kernel`` is False.  A MeetingScheduleDomain
        within ``meeting_tables``' limits takes ``sa_meeting_kernel`` (optimize/ga_meeting.py), a
        FeatureSubsetDomain with the built-in naive-Bayes evaluator within
        ``subset_tables``' limits takes ``sa_subset_kernel`` (optimize/ga_subset.py) — on a GPU by
        default, on the CPU (their host twins) only when ``use_kernel`` is True, so CPU default
        results are unchanged.  Measured against the generic path on one MI355X
        (profiles/sa_domains_bench.jsonl, 300 moves, whole runs): meetings 66 x / 53 x / 15 x faster
        at 1 / 64 / 4,096 chains, subsets 47 x / 47 x / 27 x at 4,000 rows and 4.0 x / 4.6 x / 5.6 x at
        65,536 rows for 1 / 64 / 1,024 chains.  One subset chain is one workgroup that streams every
        row once per move, so a single chain loses above 2^17 rows
        (profiles/sa_subset_cap_sweep.jsonl): past ``ga_subset.SA_ROW_CAP`` the default stays
        generic and ``use_kernel=True`` still forces the engine.  The state of a chain is explicit,
        so the engines work with ``recovery``."""
        d = self.domain
        if self.use_kernel is False or self.step != 1:
            return None
        if isinstance(d, AssignmentDomain):
            return _assign_chains(d, self.n_chains * world) if d.L <= 512 else None
        if getattr(d, "groups", None) or not (self.use_kernel is True or d.device.type == "cuda"):
            return None
        from . import ga_meeting as gm, ga_subset as gs
        tb = gm.meeting_tables(d)           # None unless a MeetingScheduleDomain within the kernel's limits
        if tb is not None and gm.sa_meeting_lds(tb["M"]) <= 64 * 1024:
            return _Chains(("sa_meeting_kernel", "sa_meeting_twin"), partial(gm.sa_meeting_init, tb),
                           lambda s: gm.ga_meeting_price(tb, s.cpu().numpy()), partial(gm.sa_meeting_advance, tb))
        if getattr(d, "loglik", None) is not None and d.loglik.dim() == 3:
            tb = gs.subset_tables(d)        # None unless a FeatureSubsetDomain with the built-in evaluator
            # one chain is one workgroup streaming every row once per move: by default up to
            # ga_subset.SA_ROW_CAP rows, where a single chain still beats the generic path
            if tb is not None and (self.use_kernel is True or tb["N"] <= gs.SA_ROW_CAP):
                return _Chains(("sa_subset_kernel", "sa_subset_host"), partial(gs.sa_subset_init, tb),
                               lambda s: gs.ga_subset_price(tb, gs.pack_masks(s.cpu().numpy()), d.device),
                               partial(gs.sa_subset_advance, tb))
        return None

    def _run_kernel(self, comm, init, engine):
        """K22 path.  Chains are GLOBAL: chain ``g`` draws Philox stream ``(seed, g)`` and starts from
        row ``g`` of one population drawn from ``seed`` alone, rank ``r`` runs chains
        ``[r * n_chains, (r + 1) * n_chains)``.  The W-rank result therefore equals one process
        running ``W * n_chains`` chains, and the checkpoint (rank 0 writes every chain) resumes at
        ANY world size: the restored chains are re-dealt by global index.  Under checkpointing the
        run is split into segments of ``segment`` moves (one launch each, same Philox counters and
        cooling schedule as one launch).  ``engine`` (:meth:`_chain_engine`) supplies the start
        solutions, their price and the launch."""
        from ..data.table import shard_range
        d = self.domain
        W, r = comm.world, comm.rank
        stats = {"better": 0, "worse_accepted": 0, "rejected": 0}
        best = bc = temp = None
        b0 = 0
        with IterationLoop("simulatedAnnealing", self.recovery, comm, device=d.device) as lp:
            _, st, meta = lp.restore(d.device)
            if st is not None:
                total = int(meta["chains"])
                a, e = shard_range(total, r, W)
                sol, cost, best, bc = (st[k][a:e].to(d.device) for k in ("sol", "cost", "best", "best_cost"))
                temp, b0 = float(meta["temp"]), int(meta["moves"])
                if r == 0:                                       # global counters: summed over ranks at the end
                    stats = dict(meta["stats"])
            else:
                if init is None:
                    total = self.n_chains * W
                    a = r * self.n_chains
                    sol = engine.start(d.device, self.n_chains, self.seed, a)
                else:
                    sol = init.to(d.device).long().clone()
                    counts = comm.all_gather(torch.tensor([sol.shape[0]])).view(-1).tolist()
                    total, a = sum(counts), sum(counts[:r])
                # the engines price with their own arithmetic: the current cost is always the kernel's
                # price of the solution, the same bits on either device
                cost = engine.cost(d.device, sol)
            seg = max(1, self.segment or -(-self.iters // 10)) if lp.enabled else max(1, self.iters)
            for b in range(b0, self.iters, seg):
                n = min(seg, self.iters - b)
                with lp.step(b // seg):
                    run = SaRun(n, self.t0, self.cooling, self.interval, self.geometric, self.max_retry, self.seed,
                                it_begin=b, temp_start=temp, chain_base=a)
                    best, bc, s, sol, cost, temp = engine.advance(d.device, sol, cost, run, best, bc)
                for k in stats:
                    stats[k] += s[k]
                if lp.enabled:
                    full = [comm.all_gather_v(x.contiguous()) for x in (sol, cost, best, bc)]
                    lp.commit(b // seg, dict(zip(("sol", "cost", "best", "best_cost"), full)),
                              {"temp": temp, "moves": b + n, "stats": self._global_stats(comm, stats),
                               "chains": total}, force=True)
        if best is None:                                   # no moves at all
            best, bc = sol.clone(), cost.clone()
        stats = self._global_stats(comm, stats)
        if engine.names:
            stats["engine"] = engine.names[0 if d.device.type == "cuda" else 1]
        return best.long(), bc, stats, a

    @staticmethod
    def _global_stats(comm, stats: dict) -> dict:
        if not comm.is_distributed:
            return dict(stats)
        v = torch.tensor([stats[k] for k in ("better", "worse_accepted", "rejected")], dtype=torch.float64)
        comm.all_reduce(v)
        return dict(zip(("better", "worse_accepted", "rejected"), (int(x) for x in v.tolist())))

    def _generic(self, sol, cost, gen, lp: IterationLoop | None = None):
        d = self.domain
        best, bc = sol.clone(), cost.clone()
        temp = self.t0
        stats = {"better": 0, "worse_accepted": 0, "rejected": 0}
        it0 = 0
        if lp is not None:
            it0, st, meta = lp.restore(d.device)
            if st is not None:
                sol, cost, best, bc = st["sol"], st["cost"], st["best"], st["best_cost"]
                gen.set_state(st["rng"])
                temp, stats = float(meta["temp"]), dict(meta["stats"])
        for it in range(it0, self.iters):
            if lp is not None:
                with lp.step(it):
                    pass
            cand, _ = d.mutate(sol, self.step, gen, self.max_retry)
            cc = d.evaluate(cand)
            delta = cc - cost
            u = torch.rand(cost.shape, generator=gen, device=cost.device)
            acc = (delta <= 0) | (u < torch.exp(-delta / max(temp, 1e-12)))
            stats["better"] += int((delta <= 0).sum())
            stats["worse_accepted"] += int((acc & (delta > 0)).sum())
            stats["rejected"] += int((~acc).sum())
            sol = torch.where(acc.view(-1, 1), cand, sol)
            cost = torch.where(acc, cc, cost)
            imp = cost < bc
            best[imp] = sol[imp]
            bc = torch.minimum(bc, cost)
            if self.interval > 0 and (it + 1) % self.interval == 0:
                temp = temp * self.cooling if self.geometric else max(self.t0 - (it + 1) * self.cooling, 1e-12)
            if lp is not None and lp.enabled:
                lp.commit(it, {"sol": sol, "cost": cost, "best": best, "best_cost": bc, "rng": gen.get_state()},
                          {"temp": temp, "stats": stats})
        return best, bc, stats


def _assign_chains(d: AssignmentDomain, total: int | None = None) -> _Chains:
    """``sa_assign_kernel`` and its twin (optimize/sa.py); the starts are rows of one population of ``total`` chains."""
    return _Chains(None, partial(sa_assign_init, d, total=total), d.evaluate, partial(sa_assign_advance, d))


def sa_assign(d: AssignmentDomain, sol: torch.Tensor, cost: torch.Tensor, iters: int, t0: float, cool: float,
              interval: int, geometric: bool, max_retry: int, seed: int, offset: int, it_begin: int = 0,
              temp_start: float | None = None, best: torch.Tensor | None = None, best_cost: torch.Tensor | None = None,
              return_state: bool = False, chain_base: int = 0):
    """Run ``sol.shape[0]`` SA chains over an assignment domain: K22 kernel on GPU, its numpy twin
    (same Philox stream, float32 arithmetic) on CPU.  Returns (best_sol, best_cost, stats)
    or, with ``return_state``, also (current_sol, current_cost, temperature) so a run split into
    segments [it_begin, it_begin + iters) (checkpoint / resume) equals one uninterrupted launch.
    Row ``p`` is global chain ``chain_base + p``: its Philox stream does not depend on the launch."""
    run = SaRun(iters, t0, cool, interval, geometric, max_retry, seed, offset, it_begin, temp_start, chain_base)
    out = _assign_chains(d).advance(sol.device, sol, cost, run, best, best_cost)
    return out if return_state else out[:3]


def local_focussed(d: SearchDomain, sols: torch.Tensor, costs: torch.Tensor, n_iter: int, gen=None):
    """Neighbours of each solution (reference = the start solution, not the walk), keep the best
    (SimulatedAnnealing.scala:199-234 / RandomSearch.localFocussedSearch :170-210): one batch of
    ``P * n_iter`` mutants."""
    P, L = sols.shape
    rep = sols.repeat_interleave(n_iter, 0)
    mut, _ = d.mutate(rep, 1, gen)
    mc = d.evaluate(mut).view(P, n_iter)
    j = mc.argmin(1)
    mb = mc[torch.arange(P), j]
    better = mb < costs
    out = sols.clone()
    out[better] = mut.view(P, n_iter, L)[torch.arange(P, device=sols.device)[better], j[better]]
    return out, torch.where(better, mb, costs)


def local_trajectory(d: SearchDomain, sols: torch.Tensor, costs: torch.Tensor, n_iter: int, gen=None,
                     fanout: int = 4):
    """Hill climb: each step samples ``fanout`` neighbours of the CURRENT solution and moves to the
    best if it improves (OptUtility.localTrajectorySearch, J/optimize/OptUtility.java:46-66)."""
    P, L = sols.shape
    cur, cc = sols.clone(), costs.clone()
    for _ in range(n_iter):
        nb, nc = local_focussed(d, cur, cc, fanout, gen)
        cur, cc = nb, nc
    return cur, cc


# ================================================================================================
# population optimisers
# ================================================================================================
class _Islands:
    """An island engine: one of the island kernels of optim.hip on a GPU, its host twin on the CPU.
    ``names`` are the (GPU, CPU) engine names of ``OptResult.stats``; ``init(n, P, seed, island_base)``
    returns the initial pools and costs; ``run(pop, cost, G, m, r, purge_first, mutate, seed,
    island_base, device, gen_base=)`` advances them."""

    def __init__(self, names, init, run):
        self.names, self.init, self.run = names, init, run

    def name(self, device) -> str:
        return self.names[0] if device.type == "cuda" else self.names[1]


class GeneticAlgorithm:
    """Island-model GA: ``islands`` independent pools advance together as one [I, pool, L] batch.

    Per generation and island: sort, take the ``mating`` best, make ``replacement`` children by
    single-point crossover of random mating pairs + mutation, keep valid children, purge the
    ``replacement`` worst (before or after adding, ``purge_first``).  Optional ring migration of
    island elites every ``migrate_every`` generations (the reference islands never exchange)."""

    def __init__(self, domain: SearchDomain, islands: int = 4, pool: int = 10, mating: int = 5, replacement: int = 5,
                 generations: int = 100, purge_first: bool = True, mutate_children: bool = True,
                 migrate_every: int = 0, seed: int = 0, comm: Comm | None = None,
                 recovery: RecoveryConfig | None = None, use_kernel: bool | None = None):
        self.d = domain
        self.use_kernel = use_kernel    # None: the island kernel (optimize/ga.py) whenever it applies
        self.recovery = recovery        # per-generation checkpoint / resume (utils/resilience)
        self.I, self.Pp, self.m, self.r, self.G = islands, pool, mating, replacement, generations
        self.purge_first, self.mutate_children, self.migrate_every = purge_first, mutate_children, migrate_every
        self.seed, self.comm = seed, comm

    @classmethod
    def from_properties(cls, domain, conf, islands: int = 1, **kw):
        """``opti.*`` keys of P/mlextra/optpopu.py:104-110 (a :class:`~avenir_amd.utils.config.Configuration`)."""
        return cls(domain, islands=islands, pool=conf.get_int("opti.pool.size")[0],
                   mating=conf.get_int("opti.mating.size")[0], replacement=conf.get_int("opti.replacement.size")[0],
                   generations=conf.get_int("opti.num.iter")[0], purge_first=conf.get_boolean("opti.purge.first")[0],
                   **kw)

    def run(self) -> OptResult:
        """Islands are GLOBAL: island ``g`` owns a generator seeded ``seed + 7919 g`` that draws its
        initial pool and every crossover / mutation of that island, and rank ``r`` runs islands
        ``[r * islands, (r + 1) * islands)``; migration is a ring over the global island order (one
        all-gather of the elites).  So the W-rank run equals one process running ``W * islands``
        islands, and the checkpoint — every island's pool, costs, history and generator state,
        written by rank 0 — resumes at ANY world size by re-dealing the islands by global index."""
        from ..data.table import shard_range
        comm = self.comm or get_comm()
        engine = self._island_engine()
        if engine is not None:
            return self._run_islands(comm, engine)
        d, Pp, L = self.d, self.Pp, self.d.L
        W, r = comm.world, comm.rank
        lp = IterationLoop("geneticAlgorithm", self.recovery, comm, device=d.device)
        g0, st, meta = lp.restore(d.device)
        if st is not None:
            total = int(meta["islands"])
            a, e = shard_range(total, r, W)
            pop, cost, hist = (st[k][a:e].to(d.device) for k in ("pop", "cost", "hist"))
            gens = []
            for i in range(a, e):
                gg = _gen(d.device, 0)
                gg.set_state(st["rng"][i].cpu().clone())
                gens.append(gg)
        else:
            total, a, e = self.I * W, r * self.I, (r + 1) * self.I
            gens = [_gen(d.device, self.seed + 7919 * i) for i in range(a, e)]
            pop = torch.stack([d.random(Pp, gg)[0] for gg in gens]).view(e - a, Pp, L)
            cost = d.evaluate(pop.view(-1, L)).view(e - a, Pp)
            hist = torch.empty((e - a, 0), dtype=cost.dtype, device=d.device)
        for g in range(g0, self.G):
            with lp.step(g):
                outs = [self._generation(pop[i:i + 1], cost[i:i + 1], gens[i]) for i in range(e - a)]
                if outs:
                    pop = torch.cat([o[0] for o in outs])
                    cost = torch.cat([o[1] for o in outs])
                    hist = torch.cat([hist, torch.cat([o[2] for o in outs]).view(-1, 1)], 1)
                if self.migrate_every and total > 1 and (g + 1) % self.migrate_every == 0:
                    pop, cost = self._migrate(comm, pop, cost, a, e)
            if lp.enabled:
                rng = torch.stack([gg.get_state() for gg in gens]) if gens else torch.empty((0, 1), dtype=torch.uint8)
                full = [comm.all_gather_v(x.contiguous()) for x in (pop, cost, hist, rng)]
                lp.commit(g, dict(zip(("pop", "cost", "hist", "rng"), full)), {"islands": total})
        lp.close()
        ha = comm.all_gather_v(hist.contiguous()) if comm.is_distributed else hist
        history = ha.min(0).values.tolist() if ha.shape[0] else []
        ii = torch.arange(e - a, device=d.device)
        bi = cost.argmin(1)
        bs, bc = pop[ii, bi], cost[ii, bi]
        b, c = _global_best(comm, bc, bs)
        return OptResult(b, c, bc, bs, history)

    def _island_engine(self):
        """The one-launch island kernel that applies to this run, or None (the generic torch path):
        no tied groups or checkpointing, pools of <= 64, LDS <= 64 KiB per island.  Assignment
        domains take ``ga_assign_kernel`` (optimize/ga.py), on the CPU its host twin.  Meeting-schedule
        domains within the kernel's limits take ``ga_meeting_kernel`` (optimize/ga_meeting.py) on a
        GPU; on the CPU its twin runs only when ``use_kernel`` is True, so CPU results are unchanged.
        Under the same rule, feature-subset domains with the built-in naive-Bayes evaluator take
        ``ga_subset_kernel`` (optimize/ga_subset.py) up to ``ga_subset.ROW_CAP`` = 2^15 data rows:
        one workgroup streams every row once per generation, so a single island is bound by one
        CU.  Measured at 1 island (churn model, 100 generations, profiles/ga_subset_cap_sweep.jsonl)
        the kernel run takes 46 ms against 66 ms at 2^15 rows and 92 ms against 69 ms at 2^16, so
        above the cap the generic path stays (with 64 islands the kernel still wins at 2^20 rows)."""
        d = self.d
        if self.use_kernel is False or getattr(d, "groups", None) or self.recovery is not None:
            return None
        from functools import partial
        from . import ga, ga_meeting as gm, ga_subset as gs
        P, r = self.Pp, self.r
        if not ga.ga_pool_ok(P, self.m, r, self.purge_first):
            return None
        if isinstance(d, AssignmentDomain):
            if ga.ga_assign_lds(P, d.L, r) > 64 * 1024 or d.V > 32767:
                return None
            return _Islands(("ga_assign_kernel", "ga_twin"), partial(ga.ga_assign_init, d), partial(ga.ga_assign_run, d))
        if self.use_kernel is True or d.device.type == "cuda":
            tb = gm.meeting_tables(d)       # None unless a MeetingScheduleDomain within the kernel's limits
            if tb is not None and gm.ga_meeting_lds(P, d.L, r) <= 64 * 1024:
                def init(n, P, seed, island_base):
                    pop = gm.ga_meeting_init(tb, n, P, seed, island_base)
                    return pop, gm.ga_meeting_price(tb, pop)
                return _Islands(("ga_meeting_kernel", "ga_meeting_twin"), init, partial(gm.ga_meeting_run, tb))
            if getattr(d, "loglik", None) is not None and d.loglik.dim() == 3 and d.loglik.shape[0] <= gs.ROW_CAP:
                tb = gs.subset_tables(d)    # None unless a FeatureSubsetDomain with the built-in evaluator
                if tb is not None and gs.ga_subset_lds(tb["N"], tb["F"], tb["C"]) <= 48 * 1024:
                    def init(n, P, seed, island_base):
                        pop = gs.ga_subset_init(tb, n, P, seed, island_base)
                        return pop, gs.ga_subset_price(tb, gs.pack_masks(pop), d.device)
                    return _Islands(("ga_subset_kernel", "ga_subset_host"), init, partial(gs.ga_subset_run, tb))
        return None

    def _run_islands(self, comm, engine) -> OptResult:
        """All of this rank's islands, G generations, in one kernel launch (per migration interval):
        islands [r * islands, (r + 1) * islands) by GLOBAL index, so the W-rank run equals one
        process running W * islands; migration (ring of elites) runs on host copies between
        launches, identically on either device.  ``engine`` supplies the initial pools and advances
        them (the kernel on the GPU, its twin on the host)."""
        d = self.d
        W, rk = comm.world, comm.rank
        a, e = rk * self.I, (rk + 1) * self.I
        total = self.I * W
        pop, cost = engine.init(e - a, self.Pp, self.seed, a)
        step = self.migrate_every if (self.migrate_every and total > 1) else self.G
        hists = []
        g = 0
        while g < self.G:
            k = min(step, self.G - g)
            pop, cost, h = engine.run(pop, cost, k, self.m, self.r, self.purge_first, self.mutate_children,
                                      self.seed, a, d.device, gen_base=g)
            hists.append(h)
            g += k
            if g < self.G and step < self.G:
                tp, tc = self._migrate(comm, torch.from_numpy(pop.astype(np.int64)), torch.from_numpy(cost), a, e)
                pop, cost = tp.numpy().astype(np.int16), tc.numpy().astype(np.float32)
        hist = torch.from_numpy(np.concatenate(hists, 1) if hists else np.zeros((e - a, 0), np.float32))
        ha = comm.all_gather_v(hist.contiguous()) if comm.is_distributed else hist
        history = ha.min(0).values.tolist() if ha.shape[0] else []
        bi = cost.argmin(1)
        ii = np.arange(e - a)
        bs = torch.from_numpy(pop[ii, bi].astype(np.int64)).to(d.device)
        bc = torch.from_numpy(cost[ii, bi]).to(d.device)
        b, c = _global_best(comm, bc, bs)
        return OptResult(b, c, bc, bs, history, {"engine": engine.name(d.device)})

    @staticmethod
    def _migrate(comm, pop, cost, a, e):
        """Ring migration over the global islands: island g's elite replaces the worst member of
        island g + 1 (mod the island count)."""
        ii = torch.arange(e - a, device=pop.device)
        bi = cost.argmin(1)
        elite, ec = pop[ii, bi], cost[ii, bi]
        ge, gc = comm.all_gather_v(elite.contiguous()), comm.all_gather_v(ec.contiguous())
        ge, gc = ge.roll(1, 0)[a:e], gc.roll(1, 0)[a:e]
        wi = cost.argmax(1)
        pop, cost = pop.clone(), cost.clone()
        pop[ii, wi] = ge.to(pop.device)
        cost[ii, wi] = gc.to(cost.device)
        return pop, cost

    def _generation(self, pop, cost, gen):
        """One generation of the islands in ``pop`` [I, pool, L] (all drawing from ``gen``).
        Returns (pop, cost, best cost at the generation's start per island)."""
        d, L = self.d, self.d.L
        I, Pp = pop.shape[0], pop.shape[1]
        ii = torch.arange(I, device=d.device).view(-1, 1)
        order = cost.argsort(1)
        pop, cost = pop[ii, order], cost[ii, order]
        first = cost[:, 0].clone()
        # children: 2x oversampled pairs from the mating list, first r valid per island
        npair = self.r
        a = (torch.rand((I, npair), generator=gen, device=d.device) * self.m).long().clamp_max(self.m - 1)
        b = (torch.rand((I, npair), generator=gen, device=d.device) * (self.m - 1)).long().clamp_max(max(self.m - 2, 0))
        b = b + (b >= a).long()
        pa, pb = pop[ii, a].view(-1, L), pop[ii, b.clamp_max(Pp - 1)].view(-1, L)
        c1, c2 = d.crossover(pa, pb, gen)
        kids = torch.cat([c1.view(I, npair, L), c2.view(I, npair, L)], 1).view(-1, L)
        if self.mutate_children:
            kids, _ = d.mutate(kids, 1, gen)
        kc = d.evaluate(kids).view(I, 2 * npair)
        kids = kids.view(I, 2 * npair, L)
        ko = kc.argsort(1)[:, : self.r]                              # best r children (valid first)
        kids, kc = kids[ii, ko], kc[ii, ko]
        if self.purge_first:
            pop = torch.cat([pop[:, : Pp - self.r], kids], 1)
            cost = torch.cat([cost[:, : Pp - self.r], kc], 1)
        else:
            allp, allc = torch.cat([pop, kids], 1), torch.cat([cost, kc], 1)
            o = allc.argsort(1)[:, :Pp]
            pop, cost = allp[ii, o], allc[ii, o]
        return pop, cost, first


class EvolutionaryOptimizer:
    """Mutation-only steady-state evolution (P/mlextra/optpopu.py:32-96), all islands at once:
    tournament-select the best of ``select`` random pool members, mutate a clone, purge the member
    with the worst ``w * cost + (1 - w) * age`` and insert the child.

    On a GPU, assignment, meeting-schedule and feature-subset domains run as ONE launch per run or
    checkpoint segment (optimize/eo.py: ``eo_assign_kernel`` / ``eo_meeting_kernel``, one island per
    lane, the pool in lane-private LDS columns; ``eo_subset_kernel``, 1 to 16 waves per island over a
    shared row tile, the pool in registers; :meth:`_island_engine`), bit-equal to a numpy twin that
    runs on the CPU with ``use_kernel=True``.  That path indexes islands GLOBALLY and keeps explicit
    state, so it does not depend on the world size and works with ``recovery``.  The torch path
    below is the CPU default, ``use_kernel=False`` and every other domain: about 15 small launches
    and a host read per iteration, one generator per rank."""

    def __init__(self, domain: SearchDomain, islands: int = 4, pool: int = 5, select: int = 3, iters: int = 100,
                 purge_cost_weight: float = 0.7, purge_age_scale: float = 1.0, seed: int = 0, comm: Comm | None = None,
                 use_kernel: bool | None = None, recovery: RecoveryConfig | None = None, segment: int | None = None):
        self.d = domain
        self.I, self.Pp, self.k, self.iters = islands, pool, select, iters
        self.w, self.age_scale, self.seed, self.comm = purge_cost_weight, purge_age_scale, seed, comm
        self.use_kernel = use_kernel    # None: the island kernel (optimize/eo.py) whenever it applies
        self.recovery = recovery        # checkpoint / resume of the kernel path (utils/resilience)
        self.segment = segment          # iterations per checkpointed segment (default iters / 10)

    @classmethod
    def from_properties(cls, domain, conf, islands: int = 1, **kw):
        """``opti.*`` keys of P/mlextra/optpopu.py:37-43 (a :class:`~avenir_amd.utils.config.Configuration`)."""
        return cls(domain, islands=islands, pool=conf.get_int("opti.pool.size")[0],
                   select=conf.get_int("opti.pool.select.size")[0], iters=conf.get_int("opti.num.iter")[0],
                   purge_cost_weight=conf.get_float("opti.purge.cost.weight")[0],
                   purge_age_scale=conf.get_float("opti.purge.age.scale")[0], **kw)

    def _island_engine(self):
        """The one-launch island kernel that applies to this run, or None (the torch path of
        :meth:`run`): no tied groups and the pool inside the frame's limits (``eo.eo_pool_ok``).  An
        AssignmentDomain (2 <= V <= 32767) takes ``eo_assign_kernel``, a MeetingScheduleDomain within
        ``meeting_tables``' limits ``eo_meeting_kernel`` — both while one island's columns fit 64 KiB
        of LDS (``eo.eo_assign_plan`` / ``eo.eo_meeting_plan``) — and a FeatureSubsetDomain with the
        built-in naive-Bayes evaluator within ``subset_tables``' limits ``eo_subset_kernel``
        (optimize/ga_subset.py): on a GPU by default, on the CPU (their host twin) only when
        ``use_kernel`` is True, so CPU default results are unchanged.  Measured against the torch
        path on one MI355X (profiles/eo_islands_bench.jsonl, benchmarks/bench_eo_islands.py: 300
        iterations, pool 5, select 3, whole runs, medians of 5): the 24 x 10 assignment 15 x / 11 x /
        6.4 x faster at 1 / 64 / 4,096 islands (30 against 464 ms, 99 ms against 1.10 s, 182 ms
        against 1.17 s), meetings (10 meetings, 20 people) 60 x / 44 x / 4.1 x (7.4 against 441 ms,
        14.1 against 615 ms, 205 against 833 ms), churn subsets 60 x / 56 x / 26 x at 4,000 rows and
        1 / 64 / 1,024 islands (4.6 against 278 ms, 5.1 against 283 ms, 11.6 against 298 ms) and
        6.3 x / 6.8 x / 6.5 x at 65,536 rows (44 against 277 ms, 46 against 310 ms, 109 against
        716 ms).  One subset island is one workgroup that streams every row once per iteration, so
        a single island stops winning at 2^18 rows (288 against 307 ms, inside the runs' spread; 578
        against 288 ms at 2^19: profiles/eo_subset_cap_sweep.jsonl): past ``ga_subset.EO_ROW_CAP`` =
        2^17 rows (147 against 326 ms) the default stays on the torch path and ``use_kernel=True``
        still forces the engine.  No other measured configuration loses, so assignments and
        meetings have no cap beyond the LDS limit.  Not measured: the kernels alone (the times
        include the host-drawn start pools, their pricing and the copies), pools above 5,
        multi-GPU runs."""
        d = self.d
        if self.use_kernel is False or getattr(d, "groups", None):
            return None
        if not (self.use_kernel is True or d.device.type == "cuda"):
            return None
        from . import eo, ga, ga_meeting as gm, ga_subset as gs
        if not eo.eo_pool_ok(self.Pp, self.k, self.w, self.age_scale, self.iters):
            return None
        if isinstance(d, AssignmentDomain):
            if not 2 <= d.V <= 32767 or eo.eo_assign_plan(self.Pp, d.L)[0] == 0:
                return None
            return _Islands(("eo_assign_kernel", "eo_assign_twin"), partial(ga.ga_assign_init, d),
                            partial(eo.eo_assign_advance, d))
        tb = gm.meeting_tables(d)           # None unless a MeetingScheduleDomain within the kernel's limits
        if tb is not None and eo.eo_meeting_plan(self.Pp, tb["M"])[0] > 0:
            def init(n, P, seed, island_base):
                pop = gm.ga_meeting_init(tb, n, P, seed, island_base)
                return pop, gm.ga_meeting_price(tb, pop)
            return _Islands(("eo_meeting_kernel", "eo_meeting_twin"), init, partial(gm.eo_meeting_advance, tb))
        if getattr(d, "loglik", None) is not None and d.loglik.dim() == 3:
            tb = gs.subset_tables(d)        # None unless a FeatureSubsetDomain with the built-in evaluator
            # one island is one workgroup streaming every row once per iteration: by default up to
            # ga_subset.EO_ROW_CAP rows
            if tb is not None and (self.use_kernel is True or tb["N"] <= gs.EO_ROW_CAP):
                def init(n, P, seed, island_base):
                    pop = gs.ga_subset_init(tb, n, P, seed, island_base)
                    return pop, gs.ga_subset_price(tb, gs.pack_masks(pop), d.device)
                return _Islands(("eo_subset_kernel", "eo_subset_host"), init, partial(gs.eo_subset_advance, tb))
        return None

    def _run_kernel(self, comm, engine) -> OptResult:
        """K22 path.  Islands are GLOBAL: island ``g`` draws Philox streams keyed by ``g`` and starts
        from the pool that ``ga_*_init`` draws for ``(seed, g)``; rank ``r`` runs islands ``[r I, (r + 1) I)``,
        so the W-rank run equals one process with ``W I`` islands.  Under checkpointing the run is cut
        into segments of ``segment`` iterations (one launch each, the same Philox counters and stamps
        as one launch); rank 0 writes every island and a resume re-deals them by global index over
        ANY world size.  ``history`` is the per-iteration minimum over all global islands, ``stats``
        the counters ``inserted`` / ``stalls`` / ``improved`` summed over ranks, and ``engine``."""
        from ..data.table import shard_range
        from .eo import EoRun
        d = self.d
        W, r = comm.world, comm.rank
        keys = ("pop", "cost", "born", "best", "best_cost", "hist")
        names = ("inserted", "stalls", "improved")
        stats = dict.fromkeys(names, 0)
        b0 = 0
        with IterationLoop("evolutionary", self.recovery, comm, device=d.device) as lp:
            _, st, meta = lp.restore("cpu")
            if st is not None:
                total = int(meta["islands"])
                a, e = shard_range(total, r, W)
                pop, cost, born, best, bc, hist = (st[k][a:e].cpu().numpy() for k in keys)
                b0 = int(meta["iters"])
                if r == 0:                                       # global counters: summed over ranks at the end
                    stats = dict(meta["stats"])
            else:
                total, a = self.I * W, r * self.I
                pop, cost = engine.init(self.I, self.Pp, self.seed, a)
                born = best = bc = None
                hist = np.zeros((self.I, 0), dtype=np.float32)
            seg = max(1, self.segment or -(-self.iters // 10)) if lp.enabled else max(1, self.iters)
            for b in range(b0, self.iters, seg):
                n = min(seg, self.iters - b)
                with lp.step(b // seg):
                    run = EoRun(n, self.k, self.w, self.age_scale, self.seed, b, a)
                    best, bc, s, pop, cost, born, h = engine.run(pop, cost, run, d.device, born, best, bc)
                hist = np.concatenate([hist, h], axis=1)
                for k in names:
                    stats[k] += s[k]
                if lp.enabled:
                    # int16 state travels as int32 (gloo has no int16)
                    full = [comm.all_gather_v(torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32 if x.dtype == np.int16
                                                                                    else x.dtype)))
                            for x in (pop, cost, born, best, bc, hist)]
                    lp.commit(b // seg, dict(zip(keys, full)),
                              {"iters": b + n, "stats": self._global_stats(comm, stats, names), "islands": total},
                              force=True)
        if best is None:                                   # no iterations at all: the first smallest-cost member
            ii, first = np.arange(pop.shape[0]), cost.argmin(1)
            best, bc = pop[ii, first], cost[ii, first]
        stats = self._global_stats(comm, stats, names)
        stats["engine"] = engine.name(d.device)
        ht = torch.from_numpy(np.ascontiguousarray(hist))
        ha = comm.all_gather_v(ht) if comm.is_distributed else ht
        history = ha.min(0).values.tolist() if ha.shape[0] else []
        bs = torch.from_numpy(np.asarray(best).astype(np.int64)).to(d.device)
        bct = torch.from_numpy(np.asarray(bc, dtype=np.float32)).to(d.device)
        b, c = _global_best(comm, bct, bs)
        return OptResult(b, c, bct, bs, history, stats)

    @staticmethod
    def _global_stats(comm, stats: dict, names) -> dict:
        if not comm.is_distributed:
            return dict(stats)
        v = torch.tensor([stats[k] for k in names], dtype=torch.float64)
        comm.all_reduce(v)
        return dict(zip(names, (int(x) for x in v.tolist())))

    def run(self) -> OptResult:
        comm = self.comm or get_comm()
        engine = self._island_engine()
        if engine is not None:
            return self._run_kernel(comm, engine)
        d, I, Pp, L = self.d, self.I, self.Pp, self.d.L
        dev = d.device
        gen = _gen(dev, self.seed + 104729 * comm.rank)
        pop, _ = d.random(I * Pp, gen)
        cost = d.evaluate(pop).view(I, Pp)
        pop = pop.view(I, Pp, L)
        born = torch.arange(Pp, device=dev).view(1, -1).repeat(I, 1)
        ii = torch.arange(I, device=dev)
        bi0 = cost.argmin(1)
        best, bc = pop[ii, bi0].clone(), cost[ii, bi0].clone()
        history = []
        for it in range(self.iters):
            sel = torch.rand((I, Pp), generator=gen, device=dev).argsort(1)[:, : self.k]
            sc = cost.gather(1, sel)
            w = sel.gather(1, sc.argmin(1, keepdim=True)).view(-1)
            child, ok = d.mutate(pop[ii, w], 1, gen)
            cc = d.evaluate(child)
            # purge: age by insertion order (older = larger), P/mlextra/opti.py purge :630-645
            rank = born.argsort(1).argsort(1)
            age = (Pp - rank).float() * self.age_scale / Pp
            fin = torch.where(torch.isfinite(cost), cost, torch.full_like(cost, 1e30))
            aggr = self.w * fin + (1 - self.w) * age
            wi = aggr.argmax(1)
            upd = ok
            pop[ii[upd], wi[upd]] = child[upd]
            cost[ii[upd], wi[upd]] = cc[upd]
            born[ii[upd], wi[upd]] = Pp + it
            imp = upd & (cc < bc)
            best[imp], bc[imp] = child[imp], cc[imp]
            history.append(float(bc.min()))
        b, c = _global_best(comm, bc, best)
        return OptResult(b, c, bc, best, history)


class RandomSearch:
    """Random multi-start: ``n`` random solutions (sharded over ranks), global best by all-gather,
    then optional ``focussed`` or ``trajectory`` local search (S/optimize/RandomSearch.scala)."""

    def __init__(self, domain: SearchDomain, n: int = 1024, local: str | None = "focussed", local_iters: int = 50,
                 seed: int = 0, comm: Comm | None = None, top_k: int = 10):
        self.d, self.n, self.local, self.local_iters, self.seed, self.comm, self.top_k = \
            domain, n, local, local_iters, seed, comm, top_k

    def run(self) -> OptResult:
        comm = self.comm or get_comm()
        d = self.d
        gen = _gen(d.device, self.seed + 31337 * comm.rank)
        n_local = self.n // comm.world + (1 if comm.rank < self.n % comm.world else 0)
        sol, _ = d.random(max(n_local, 1), gen)
        cost = d.evaluate(sol)
        b, c = _global_best(comm, cost, sol)
        if self.local:
            bb, cc = b.view(1, -1).to(d.device), torch.tensor([c], device=d.device)
            fn = local_focussed if self.local == "focussed" else local_trajectory
            bb, cc = fn(d, bb, cc, self.local_iters, gen)
            # every rank searched its own neighbourhood: take the best again
            b, c = _global_best(comm, cc, bb)
        k = min(self.top_k, cost.numel())
        o = cost.argsort()[:k]
        return OptResult(b, c, cost[o], sol[o])


class TabuSearch:
    """Batched tabu search over an :class:`AssignmentDomain`: every iteration scores the FULL
    single-reassignment neighbourhood ``[P, L, V]`` in closed form (cost delta from the table,
    validity of every move via one ``conflict @ occupancy`` GEMM), masks tabu moves unless they
    beat the best (aspiration), and takes the best admissible move; reversing a move is tabu for
    ``tenure`` iterations (TabuSearchDomain purge, J/optimize/TabuSearchDomain.java:54-66).

    On a GPU the whole run is one launch of ``tabu_assign_kernel`` (optimize/tabu.py: one chain per
    wave, the tabu table and the blocked counts of every cell in LDS) whenever the tables fit its
    LDS (:meth:`_chain_engine`); its numpy twin, which it equals bit for bit, runs on the CPU
    with ``use_kernel=True``.  The torch path above is the CPU default and ``use_kernel=False``."""

    def __init__(self, domain: AssignmentDomain, n_chains: int = 8, iters: int = 200, tenure: int = 7, seed: int = 0,
                 comm: Comm | None = None, use_kernel: bool | None = None):
        self.d, self.P, self.iters, self.tenure, self.seed, self.comm = domain, n_chains, iters, tenure, seed, comm
        self.use_kernel = use_kernel

    def _chain_engine(self) -> str | None:
        """``tabu_assign_kernel`` / ``tabu_assign_twin`` when the one-launch engine applies, or None (the
        generic torch path): an AssignmentDomain whose tables fit the kernel's LDS
        (``tabu.tabu_assign_lds`` <= 64 KiB, V <= 32767) — on a GPU by default, on the CPU (the
        twin) only when ``use_kernel`` is True, so CPU default results are unchanged.  Measured on
        one MI355X against the generic path (profiles/tabu_assign_bench.jsonl, 24 x 10 cells, 200
        iterations, whole runs): 54 x / 22 x / 6.3 x faster at 16 / 1,024 / 16,384 chains; at 16
        chains no size up to the LDS limit loses (profiles/tabu_assign_cap_sweep.jsonl: 8.6 x at
        160 x 48), so the dispatch has no size cap."""
        from . import tabu as tb
        d = self.d
        if self.use_kernel is False or not isinstance(d, AssignmentDomain):
            return None
        if not (self.use_kernel is True or d.device.type == "cuda"):
            return None
        if d.V > 32767 or tb.tabu_assign_lds(d.L, d.V) > tb.LDS_LIMIT or self.iters + self.tenure >= 2 ** 31:
            return None
        return "tabu_assign_kernel" if d.device.type == "cuda" else "tabu_assign_twin"

    def _run_kernel(self, comm, engine: str) -> OptResult:
        """Chains are GLOBAL: rank ``r`` runs chains ``[r n, (r + 1) n)`` of one population of ``W n``
        start solutions drawn from the seed alone, so the W-rank run equals one process with
        ``W n`` chains.  The population is drawn and priced whole on the host, then cut: both
        devices and every world size start from the same bits (a torch reduction may round
        differently for another batch shape)."""
        from .tabu import TabuRun, tabu_assign_advance
        d, n = self.d, self.P
        W, r = comm.world, comm.rank
        host = d if d.device.type == "cpu" else d.to("cpu")
        pop = sa_assign_init(host, W * n, self.seed, 0, total=W * n)
        sol, cost = pop[r * n:(r + 1) * n], host.evaluate(pop)[r * n:(r + 1) * n]
        run = TabuRun(self.iters, self.tenure, 0, r * n)
        best, bc, stats, _, _, _, hist = tabu_assign_advance(d, sol.to(d.device), cost.to(d.device), run, d.device)
        best, bc, hist = (torch.as_tensor(x) for x in (best, bc, hist))
        if comm.is_distributed:
            v = torch.tensor([stats[k] for k in ("moves", "stalls", "aspirated")], dtype=torch.float64)
            comm.all_reduce(v)
            stats = dict(zip(("moves", "stalls", "aspirated"), (int(x) for x in v.tolist())))
        ha = comm.all_gather_v(hist.cpu().contiguous()) if comm.is_distributed else hist
        history = ha.min(0).values.tolist() if ha.shape[0] else []
        best, bc = best.long().to(d.device), bc.to(d.device)
        b, c = _global_best(comm, bc, best)
        return OptResult(b, c, bc, best, history, {**stats, "engine": engine})

    def run(self) -> OptResult:
        comm = self.comm or get_comm()
        d = self.d
        engine = self._chain_engine()
        if engine is not None:
            return self._run_kernel(comm, engine)
        dev, L, V, P = d.device, d.L, d.V, self.P
        gen = _gen(dev, self.seed + 15485863 * comm.rank)
        sol, _ = d.random(P, gen)
        cost = d.evaluate(sol)
        best, bc = sol.clone(), cost.clone()
        tabu = torch.full((P, L, V), -1, dtype=torch.long, device=dev)
        rows = torch.arange(P, device=dev)
        conf = None if d.conflict is None else d.conflict.float()
        history = []
        for it in range(self.iters):
            delta = d.neighbourhood_delta(sol)                                   # [P, L, V]
            occ = torch.nn.functional.one_hot(sol, V).float()                    # [P, L, V]
            bad = torch.zeros((P, L, V), dtype=torch.bool, device=dev)
            if conf is not None:
                bad = torch.einsum("lj,pjv->plv", conf, occ) > 0
            bad |= occ.bool()                                                    # staying put is not a move
            new_cost = cost.view(-1, 1, 1) + delta
            is_tabu = tabu > it
            admissible = ~bad & (~is_tabu | (new_cost < bc.view(-1, 1, 1)))
            score = torch.where(admissible, new_cost, torch.full_like(new_cost, float("inf"))).reshape(P, -1)
            flat = score.argmin(1)
            has = torch.isfinite(score[rows, flat])
            l, v = flat // V, flat % V
            old = sol[rows, l]
            tabu[rows[has], l[has], old[has]] = it + self.tenure
            sol[rows[has], l[has]] = v[has]
            cost = torch.where(has, score[rows, flat], cost)
            imp = cost < bc
            best[imp], bc[imp] = sol[imp], cost[imp]
            history.append(float(bc.min()))
        b, c = _global_best(comm, bc, best)
        return OptResult(b, c, bc, best, history)


# ================================================================================================
# Bayesian optimisation (continuous box) — P/mlextra/optsolo.py:91-175, finished
# ================================================================================================
class BayesianOptimizer:
    """GP (RBF kernel, Cholesky) surrogate with ``pi`` / ``ei`` / ``lcb`` acquisition maximised over
    ``acq_samples`` random candidates per step; ``cost_fn(x [n, d]) -> [n]`` is vectorised."""

    def __init__(self, cost_fn: Callable, lo: Sequence[float], hi: Sequence[float], n_init: int = 20, iters: int = 30,
                 acq: str = "ei", acq_samples: int = 2048, lcb_mult: float = 2.0, length_scale: float = 0.2,
                 noise: float = 1e-6, seed: int = 0, device="cpu"):
        self.f = cost_fn
        self.lo = torch.tensor(lo, dtype=torch.float64, device=device)
        self.hi = torch.tensor(hi, dtype=torch.float64, device=device)
        self.n_init, self.iters, self.acq, self.ns, self.kappa = n_init, iters, acq, acq_samples, lcb_mult
        self.ls, self.noise, self.seed, self.device = length_scale, noise, seed, torch.device(device)

    def _k(self, a, b):
        d2 = ((a.unsqueeze(1) - b.unsqueeze(0)) ** 2).sum(2)
        return torch.exp(-0.5 * d2 / self.ls ** 2)

    def run(self) -> OptResult:
        g = _gen(self.device, self.seed)
        D = self.lo.numel()
        span = self.hi - self.lo
        X = torch.rand((self.n_init, D), generator=g, device=self.device, dtype=torch.float64)
        y = torch.as_tensor(self.f(self.lo + X * span), device=self.device).double().view(-1)
        hist = []
        for _ in range(self.iters):
            mu_y, sd_y = y.mean(), y.std().clamp_min(1e-12)
            yn = (y - mu_y) / sd_y
            K = self._k(X, X) + self.noise * torch.eye(X.shape[0], device=self.device, dtype=torch.float64)
            Lc = torch.linalg.cholesky(K + 1e-9 * torch.eye(X.shape[0], device=self.device, dtype=torch.float64))
            alpha = torch.cholesky_solve(yn.view(-1, 1), Lc)
            C = torch.rand((self.ns, D), generator=g, device=self.device, dtype=torch.float64)
            Ks = self._k(C, X)
            mu = (Ks @ alpha).view(-1)
            v = torch.cholesky_solve(Ks.T, Lc)
            var = (1.0 - (Ks * v.T).sum(1)).clamp_min(1e-12)
            sd = var.sqrt()
            best = yn.min()
            z = (best - mu) / sd
            nrm = torch.distributions.Normal(0.0, 1.0)
            if self.acq == "pi":
                a = nrm.cdf(z)
            elif self.acq == "ei":
                a = (best - mu) * nrm.cdf(z) + sd * torch.exp(nrm.log_prob(z))
            elif self.acq == "lcb":
                a = -(mu - self.kappa * sd)
            else:
                raise ValueError(self.acq)
            xn = C[int(a.argmax())].view(1, -1)
            yv = torch.as_tensor(self.f(self.lo + xn * span), device=self.device).double().view(-1)
            X, y = torch.cat([X, xn]), torch.cat([y, yv])
            hist.append(float(y.min()))
        i = int(y.argmin())
        return OptResult((self.lo + X[i] * span), float(y[i]), y, self.lo + X * span, hist)


# ================================================================================================
# hyper-parameter search (P/supv/pasearch.py)
# ================================================================================================
def parameter_search(space: dict[str, Sequence], score_fn: Callable[[dict], float], strategy: str = "random",
                     n_iter: int = 20, seed: int = 0, t0: float = 1.0, cooling: float = 0.9,
                     comm: Comm | None = None) -> tuple[dict, float, list]:
    """Search a discrete hyper-parameter grid minimising ``score_fn(params)``.

    ``guided``: coordinate-wise sweeps (GuidedParameterSearch); ``random``: random grid points
    (RandomParameterSearch); ``sa``: simulated annealing over grid neighbours
    (SimulatedAnnealingParameterSearch).  Each evaluation trains a model, so this runs on the host
    and the models themselves use the device."""
    names = list(space)
    rng = np.random.default_rng(seed)
    cache: dict = {}

    def ev(idx):
        key = tuple(idx)
        if key not in cache:
            cache[key] = float(score_fn({n: space[n][i] for n, i in zip(names, idx)}))
        return cache[key]

    hist = []
    if strategy == "guided":
        cur = [0] * len(names)
        best = ev(cur)
        for _ in range(max(1, n_iter // max(1, sum(len(space[n]) for n in names)))):
            for k, n in enumerate(names):
                for i in range(len(space[n])):
                    cand = cur.copy()
                    cand[k] = i
                    s = ev(cand)
                    if s < best:
                        best, cur = s, cand
                    hist.append(best)
    elif strategy == "random":
        cur, best = None, float("inf")
        cands = [[int(rng.integers(len(space[n]))) for n in names] for _ in range(n_iter)]
        if comm is not None and comm.is_distributed:
            # the candidates are independent, so every rank trains its share (one
            # trial per GPU) and the scores are all-gathered; the walk below then reads the cache
            todo = sorted({tuple(c) for c in cands}, key=lambda c: cands.index(list(c)))
            mine = {c: float(score_fn({n: space[n][i] for n, i in zip(names, c)}))
                    for c in todo[comm.rank::comm.world]}
            for part in comm.all_gather_object(mine):
                cache.update(part)
        for cand in cands:
            s = ev(cand)
            if s < best:
                best, cur = s, cand
            hist.append(best)
    elif strategy == "sa":
        cur = [int(rng.integers(len(space[n]))) for n in names]
        cs = ev(cur)
        best, bcur, temp = cs, cur, t0
        for _ in range(n_iter):
            cand = cur.copy()
            k = int(rng.integers(len(names)))
            if len(space[names[k]]) > 1:
                cand[k] = (cand[k] + int(rng.choice([-1, 1]))) % len(space[names[k]])
            s = ev(cand)
            if s < cs or math.exp((cs - s) / max(temp, 1e-12)) > rng.random():
                cur, cs = cand, s
                if s < best:
                    best, bcur = s, cand
            temp *= cooling
            hist.append(best)
        cur = bcur
    else:
        raise ValueError(strategy)
    return {n: space[n][i] for n, i in zip(names, cur)}, best, hist
