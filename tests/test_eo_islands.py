"""Evolutionary-optimiser islands (optimize/eo.py) over assignment domains: the frame's numpy twin —
segments, global island indexing, the branches by its own counters, invariants, the sampler and the
purge policies, runs with nothing to insert, edge shapes — the dispatch, the LDS plan, the world size,
recovery and quality of ``EvolutionaryOptimizer`` on the CPU; ``eo_assign_kernel`` against the twin (exact
in every output), segmented launches, the class on both devices and the binding's validation on the GPU."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from avenir_amd.optimize import (AssignmentDomain, CallbackDomain, EoRun, EvolutionaryOptimizer, TaskScheduleSearch,
                                 eo_assign_advance, eo_assign_reference)
from avenir_amd.optimize import eo as E
from avenir_amd.optimize.ga import ga_price
from tests._dist import run_world, run_world_outcome
from tests._eo import assert_same, assign_start, check_invariants, random_assignment, segments


def _price(d):
    conf = None if d.conflict is None else d.conflict.numpy()
    if conf is not None:
        conf = np.triu(conf, 1) | np.triu(conf, 1).T
    return lambda s: ga_price(d.cost_table.numpy(), conf, d.invalid_cost, s)


def _plain(L, V, seed=1):
    g = torch.Generator().manual_seed(seed)
    return AssignmentDomain(torch.rand((L, V), generator=g) * 100, None, invalid_cost=1e3)


@functools.lru_cache(maxsize=None)
def _branch_run():
    """The 24 x 10 assignment at 15 % conflicts: P 10, select 3, 8 islands, 300 iterations."""
    d = random_assignment(24, 10, seed=0, density=0.15)
    pop, cost = assign_start(d, 8, 10, 0)
    trace = {}
    return d, pop, cost, eo_assign_reference(d, pop, cost, EoRun(300, 3, 0.7, 1.0, 0), trace=trace), trace


# ---- CPU ---------------------------------------------------------------------------------------
def test_twin_segments_equal_one_run_and_invariants_hold():
    d, pop, cost, one, _ = _branch_run()
    twin = functools.partial(eo_assign_reference, d)
    cut = segments(twin, pop, cost, EoRun(300, 3, 0.7, 1.0, 0), 70, functools.partial(check_invariants, _price(d), 10))
    assert_same(cut, one)
    assert one[0].dtype == np.int16 and one[3].dtype == np.int16 and one[5].dtype == np.int32
    assert one[1].dtype == np.float32 and one[6].shape == (8, 300)
    check_invariants(_price(d), 10, (pop, cost, None), one)


def test_one_slot_changes_per_inserted_iteration():
    d = random_assignment(24, 10, seed=0, density=0.15)
    pop, cost = assign_start(d, 8, 10, 0)
    twin = functools.partial(eo_assign_reference, d)
    run = EoRun(40, 3, 0.7, 1.0, 0)
    cut = segments(twin, pop, cost, run, 1, functools.partial(check_invariants, _price(d), 10))
    assert_same(cut, twin(pop, cost, run))
    assert cut[2]["stalls"] > 0 and cut[2]["inserted"] > 0


def test_island_indexing_is_global():
    """Islands [3, 8) run alone equal rows 3..7 of islands [0, 8), starts included."""
    d, pop, cost, full, _ = _branch_run()
    part_pop, part_cost = assign_start(d, 5, 10, 0, 3)
    assert np.array_equal(part_pop, pop[3:]) and np.array_equal(part_cost, cost[3:])
    part = eo_assign_reference(d, part_pop, part_cost, EoRun(300, 3, 0.7, 1.0, 0, 0, 3))
    for i in (0, 1, 3, 4, 5, 6):
        assert np.array_equal(full[i][3:], part[i]), i


def test_every_branch_is_taken():
    _, _, _, out, trace = _branch_run()
    st = out[2]
    print(st, "tied tournaments", trace["tied"])
    assert st["inserted"] > 0 and st["stalls"] > 0 and st["improved"] > 0 and trace["tied"] > 0
    assert st["inserted"] + st["stalls"] == 8 * 300 and st["improved"] <= st["inserted"]


def _single_steps(d, pop, cost, run):
    """The run one iteration at a time: per iteration (state before, trace, state after)."""
    state, steps = {}, []
    for it in range(run.iters):
        trace = {}
        out = eo_assign_reference(d, pop, cost, EoRun(1, run.select, run.w, run.age_scale, run.seed, it), trace=trace,
                                  **state)
        born = state.get("born", np.broadcast_to(np.arange(pop.shape[1], dtype=np.int32), cost.shape))
        steps.append(((pop, cost, born), trace, out))
        pop, cost = out[3], out[4]
        state = {"born": out[5], "best": out[0], "best_cost": out[1]}
    return steps


def test_sampler_and_purge_policies():
    d = random_assignment(24, 10, seed=0, density=0.15)
    pop, cost = assign_start(d, 6, 10, 3)
    ar = np.arange(6)
    # select = P always picks the pool's best (the first draw among equals)
    for (_, c0, _), trace, _ in _single_steps(d, pop, cost, EoRun(40, 10, 0.7, 1.0, 3)):
        ins = trace["winner"][:, 0] >= 0
        assert np.array_equal(c0[ar[ins], trace["winner"][ins, 0]], c0.min(1)[ins])
        assert (trace["picked"] == 1).all()
    # w = 1 purges the costliest, w = 0 the oldest: the pool is a FIFO
    for (_, c0, _), trace, _ in _single_steps(d, pop, cost, EoRun(40, 3, 1.0, 1.0, 3)):
        ins = trace["victim"][:, 0] >= 0
        assert np.array_equal(c0[ar[ins], trace["victim"][ins, 0]], c0.max(1)[ins])
    fifo = _single_steps(d, pop, cost, EoRun(40, 3, 0.0, 1.0, 3))
    for (_, _, b0), trace, _ in fifo:
        ins = trace["victim"][:, 0] >= 0
        assert np.array_equal(b0[ar[ins], trace["victim"][ins, 0]], b0.min(1)[ins])
    # over a fixed seed every slot is picked with frequency k / P within 5 binomial standard deviations
    trace = {}
    eo_assign_reference(d, *assign_start(d, 8, 10, 0), EoRun(300, 3, 0.7, 1.0, 0), trace=trace)
    n, p = 8 * 300, 3 / 10
    picked = trace["picked"].sum(0)
    assert picked.sum() == n * 3 and (np.abs(picked - n * p) <= 5 * np.sqrt(n * p * (1 - p))).all(), picked


def test_nothing_to_insert():
    """5 x 3 at 60 % conflicts: every start member is invalid and no single move repairs one."""
    d = random_assignment(5, 3, seed=0, density=0.6)
    pop, cost = assign_start(d, 64, 10, 0)
    assert (cost == np.float32(d.invalid_cost)).all()
    best, bc, st, p2, c2, born, hist = eo_assign_reference(d, pop, cost, EoRun(200, 3, 0.7, 1.0, 0))
    assert st == {"inserted": 0, "stalls": 64 * 200, "improved": 0}
    assert np.array_equal(p2, pop) and np.array_equal(c2, cost) and np.array_equal(born, np.tile(np.arange(10), (64, 1)))
    assert (hist == np.float32(d.invalid_cost)).all() and np.array_equal(best, pop[:, 0])


def _edge(name):
    """(domain, pool, costs, EoRun) of an edge shape."""
    if name == "P2-select1":
        d = random_assignment(8, 5, seed=1, density=0.3)
        return (d, *assign_start(d, 5, 2, 4), EoRun(60, 1, 0.7, 1.0, 4))
    if name == "P64-select64":
        d = random_assignment(8, 5, seed=1, density=0.3)
        return (d, *assign_start(d, 3, 64, 4), EoRun(40, 64, 0.7, 1.0, 4))
    if name == "L1":
        d = random_assignment(1, 5, seed=1, density=0.3)
        return (d, *assign_start(d, 4, 5, 4), EoRun(40, 3, 0.7, 1.0, 4))
    if name == "no-conflict-no-swap":
        d = _plain(6, 4)
        d.swap_moves = False
        return (d, *assign_start(d, 4, 5, 4), EoRun(40, 3, 0.5, 2.0, 4))
    if name == "V2":
        d = random_assignment(12, 2, seed=1, density=0.1)
        return (d, *assign_start(d, 4, 6, 4), EoRun(40, 2, 0.7, 1.0, 4))
    raise KeyError(name)


_EDGES = ("P2-select1", "P64-select64", "L1", "no-conflict-no-swap", "V2")


@pytest.mark.parametrize("name", _EDGES)
def test_edge_shapes(name):
    d, pop, cost, run = _edge(name)
    one = eo_assign_reference(d, pop, cost, run)
    check_invariants(_price(d), pop.shape[1], (pop, cost, None), one)
    assert_same(segments(functools.partial(eo_assign_reference, d), pop, cost, run, 17), one)
    assert one[2]["inserted"] > 0
    if name == "L1":
        assert np.abs(one[1] - d.cost_table.numpy().min()).max() <= 1e-4


def test_state_is_checked():
    d = random_assignment(8, 5, seed=1, density=0.3)
    pop, cost = assign_start(d, 2, 4, 0)
    with pytest.raises(ValueError):
        eo_assign_reference(d, pop, cost, EoRun(3, 5))                       # select > P
    with pytest.raises(ValueError):
        eo_assign_reference(d, pop, cost, EoRun(3, 2, it_begin=2 ** 31 - 6))  # the counter bound
    with pytest.raises(ValueError):
        eo_assign_reference(d, pop, cost, EoRun(3, 2), born=np.zeros((2, 4), np.int32))
    with pytest.raises(ValueError):
        eo_assign_reference(d, pop, cost, EoRun(3, 2, w=1.5))
    bad = pop.copy()
    bad[1, 2, 3] = d.V
    with pytest.raises(ValueError):
        eo_assign_advance(d, bad, cost, EoRun(3, 2), "cpu")
    big = np.zeros((1, 65, 8), np.int16)
    with pytest.raises(ValueError):
        eo_assign_reference(d, big, np.zeros((1, 65), np.float32), EoRun(3, 2))


def test_dispatch_on_the_cpu():
    d = random_assignment(8, 5, seed=1, density=0.3)
    kw = dict(islands=4, pool=5, select=3, iters=20, seed=1)
    assert EvolutionaryOptimizer(d, **kw)._island_engine() is None
    assert EvolutionaryOptimizer(d, use_kernel=False, **kw)._island_engine() is None
    default = EvolutionaryOptimizer(d, **kw).run()
    assert "engine" not in default.stats
    res = EvolutionaryOptimizer(d, use_kernel=True, **kw).run()
    assert res.stats["engine"] == "eo_assign_twin"
    assert res.stats["inserted"] + res.stats["stalls"] == 4 * 20 and len(res.history) == 20
    assert res.costs.shape == (4,) and res.solutions.shape == (4, 8) and res.best_cost == float(res.costs.min())
    assert float(d.cost(res.best.view(1, -1))[0]) == pytest.approx(res.best_cost, rel=1e-5)

    class Obj:
        def evaluate(self, row):
            return float(sum(row))
    cb = CallbackDomain(Obj(), [[0, 1, 2]] * 4)
    assert EvolutionaryOptimizer(cb, use_kernel=True, **kw)._island_engine() is None
    grouped = random_assignment(8, 5, seed=1, density=0.3)
    grouped.groups = [[0, 1]]
    assert EvolutionaryOptimizer(grouped, use_kernel=True, **kw)._island_engine() is None
    # outside the frame's limits: the torch path even when asked for the kernel
    for over in (dict(pool=65), dict(pool=5, select=6), dict(purge_cost_weight=1.5)):
        assert EvolutionaryOptimizer(d, use_kernel=True, **{**kw, **over})._island_engine() is None
    long = random_assignment(600, 3, seed=1, density=0.0)
    assert E.eo_assign_plan(64, 600) == (0, E.eo_island_bytes(64, 600)) and E.eo_island_bytes(64, 600) > E.LDS_LIMIT
    assert EvolutionaryOptimizer(long, use_kernel=True, **{**kw, "pool": 64})._island_engine() is None
    assert EvolutionaryOptimizer(long, use_kernel=True, **kw)._island_engine() is not None


def test_from_properties():
    from avenir_amd.utils.config import Configuration
    conf = Configuration({"opti.pool.size": "7", "opti.pool.select.size": "4", "opti.num.iter": "30",
                          "opti.purge.cost.weight": "0.6", "opti.purge.age.scale": "2.0"}, {})
    eo = EvolutionaryOptimizer.from_properties(random_assignment(8, 5), conf, islands=3, use_kernel=True, seed=2)
    assert (eo.I, eo.Pp, eo.k, eo.iters, eo.w, eo.age_scale, eo.seed) == (3, 7, 4, 30, 0.6, 2.0, 2)
    assert eo.run().stats["engine"] == "eo_assign_twin"


def test_lds_plan():
    # 4 P costs + 2 P ranks + 2 P L pool + 2 L clone bytes per island; IW = the largest power of two that fits 64 KiB
    assert E.eo_island_bytes(10, 24) == 40 + 20 + 480 + 48
    assert E.eo_assign_plan(10, 24) == (64, 64 * 588)
    assert E.eo_assign_plan(64, 96) == (4, 4 * (256 + 128 + 12288 + 192))
    assert E.eo_assign_plan(5, 200) == (16, 16 * (20 + 10 + 2000 + 400))
    assert E.eo_assign_plan(64, 500)[0] == 1 and E.eo_assign_plan(64, 510)[0] == 0
    for P, L in ((2, 1), (64, 1), (10, 24), (64, 96), (64, 500), (33, 77)):
        iw, lds = E.eo_assign_plan(P, L)
        assert iw in (64, 32, 16, 8, 4, 2, 1) and lds == iw * E.eo_island_bytes(P, L) <= E.LDS_LIMIT
        assert iw == 64 or 2 * iw * E.eo_island_bytes(P, L) > E.LDS_LIMIT
    assert E.eo_meeting_plan(5, 10) == (64, 3008 + 64 * (20 + 80 + 10 + 300 + 60))


def _eo_world(rank, world, n):
    from avenir_amd.parallel.comm import get_comm
    d = random_assignment(8, 5, seed=1, density=0.3)
    r = EvolutionaryOptimizer(d, islands=n, pool=6, select=3, iters=40, seed=5, comm=get_comm(), use_kernel=True).run()
    return r.best.numpy(), r.best_cost, r.costs.numpy(), r.solutions.numpy(), r.history, r.stats


def test_two_ranks_equal_one_process():
    got = run_world(_eo_world, 2, 3)
    d = random_assignment(8, 5, seed=1, density=0.3)
    one = EvolutionaryOptimizer(d, islands=6, pool=6, select=3, iters=40, seed=5, use_kernel=True).run()
    assert np.array_equal(np.concatenate([g[2] for g in got]), one.costs.numpy())
    assert np.array_equal(np.concatenate([g[3] for g in got]), one.solutions.numpy())
    for best, best_cost, _, _, history, stats in got:
        assert np.array_equal(best, one.best.numpy()) and best_cost == one.best_cost
        assert history == one.history and stats == one.stats


def _eo_recovery(rank, world, ckdir):
    from avenir_amd.utils.resilience import RecoveryConfig
    d = random_assignment(8, 5, seed=1, density=0.3)
    r = EvolutionaryOptimizer(d, islands=8 // world, pool=6, select=3, iters=60, seed=1, use_kernel=True,
                              recovery=RecoveryConfig(ckdir), segment=10).run()
    return r.best_cost, r.best.tolist(), r.costs.tolist(), r.solutions.tolist(), r.history, r.stats


def test_fault_then_fresh_resume_equals_uninterrupted(tmp_path):
    """The pattern of tests/test_recovery.py: rank 1 exits at the start of segment 3, fresh processes
    resume from the checkpoint and end where the uninterrupted run ends — which is the run without
    checkpoints, and at another world size too."""
    fault = {"AVMI_FAULT_RANK": "1", "AVMI_FAULT_ITER": "3", "AVMI_FAULT_MODE": "exit"}
    clean, errs, codes = run_world_outcome(_eo_recovery, 2, str(tmp_path / "clean"))
    assert not errs and codes == [0, 0], errs
    assert clean[0][5]["engine"] == "eo_assign_twin"
    ck = str(tmp_path / "faulty")
    res, errs, codes = run_world_outcome(_eo_recovery, 2, ck, env=fault, timeout=90)
    assert codes[1] == 17 and len(res) < 2, (codes, errs)
    assert list((tmp_path / "faulty").glob("*.ckpt")), "no checkpoint was committed before the fault"
    resumed, errs, codes = run_world_outcome(_eo_recovery, 2, ck)
    assert not errs and codes == [0, 0], errs
    assert resumed == clean
    d = random_assignment(8, 5, seed=1, density=0.3)
    one = EvolutionaryOptimizer(d, islands=8, pool=6, select=3, iters=60, seed=1, use_kernel=True).run()
    assert one.best_cost == clean[0][0] and one.history == clean[0][4]
    assert one.costs.tolist() == clean[0][2] + clean[1][2]
    assert {k: v for k, v in one.stats.items()} == clean[0][5]


@pytest.fixture
def task_domain(ref_resource):
    return TaskScheduleSearch.from_json(ref_resource("taskSched.json"))


def test_twin_reaches_the_task_schedule_bound(task_domain):
    d = task_domain
    lb = float(d.cost_table.min(1).values.mean())
    r = EvolutionaryOptimizer(d, islands=8, pool=10, select=3, iters=300, use_kernel=True).run()
    print("twin", r.best_cost - lb)
    assert r.stats["engine"] == "eo_assign_twin" and r.best_cost <= lb + 3.0
    assert bool(d.valid(r.best.view(1, -1))) and r.history[-1] == r.best_cost


# ---- GPU ---------------------------------------------------------------------------------------
def _case(name):
    """(domain, pool, costs, EoRun) of a kernel case."""
    if name in _EDGES:
        return _edge(name)
    if name.startswith("islands-"):     # a partial wave, a tail, several workgroups
        n = int(name.split("-")[1])
        d = random_assignment(24, 10, seed=0, density=0.15)
        return (d, *assign_start(d, n, 10, 0), EoRun(120, 3, 0.7, 1.0, 0))
    if name == "island-base":
        d = random_assignment(24, 10, seed=0, density=0.15)
        return (d, *assign_start(d, 5, 10, 0, 3), EoRun(300, 3, 0.7, 1.0, 0, 0, 3))
    if name == "P64xL96":               # 4 islands per wave: 12 islands are 3 workgroups, 13 a tail
        d = random_assignment(96, 12, seed=2, density=0.02)
        return (d, *assign_start(d, 13, 64, 1), EoRun(60, 5, 0.7, 1.0, 1))
    if name == "P5xL200":               # 16 islands per wave
        d = random_assignment(200, 30, seed=2, density=0.005)
        return (d, *assign_start(d, 20, 5, 1), EoRun(60, 3, 0.7, 1.0, 1))
    if name == "nothing-to-insert":
        d = random_assignment(5, 3, seed=0, density=0.6)
        return (d, *assign_start(d, 64, 10, 0), EoRun(200, 3, 0.7, 1.0, 0))
    if name == "last-iteration":        # it_begin + iters + P = 2^31 - 1
        d = random_assignment(8, 5, seed=1, density=0.3)
        return (d, *assign_start(d, 4, 6, 4), EoRun(3, 3, 0.7, 1.0, 4, 2 ** 31 - 10))
    raise KeyError(name)


_CASES = _EDGES + ("islands-1", "islands-63", "islands-65", "islands-130", "island-base", "P64xL96", "P5xL200",
                   "nothing-to-insert", "last-iteration")


@pytest.mark.gpu
@pytest.mark.parametrize("name", _CASES)
def test_kernel_bit_equal_to_twin(cuda, name):
    d, pop, cost, run = _case(name)
    want = eo_assign_reference(d, pop, cost, run)
    got = eo_assign_advance(d.to(cuda), pop, cost, run, cuda)
    assert_same(got, want)
    if name == "islands-130":
        assert min(want[2].values()) > 0
    if name == "nothing-to-insert":
        assert want[2]["stalls"] == 64 * 200
    if name == "island-base":
        full = _branch_run()[3]                                              # rows 3..7 of islands [0, 8)
        for i in (0, 1, 3, 4, 5, 6):
            assert np.array_equal(full[i][3:], got[i]), i


@pytest.mark.gpu
def test_segmented_launches_equal_one_launch_and_the_twin(cuda):
    d = random_assignment(24, 10, seed=0, density=0.15)
    pop, cost = assign_start(d, 70, 10, 0)
    dc = d.to(cuda)
    kernel = lambda p, c, run, **st: eo_assign_advance(dc, p, c, run, cuda, **st)
    run = EoRun(120, 3, 0.7, 1.0, 0)
    one = kernel(pop, cost, run)
    assert_same(segments(kernel, pop, cost, run, 50), one)
    assert_same(one, eo_assign_reference(d, pop, cost, run))
    # resident state: tensors on the GPU in, tensors on the GPU out
    res = kernel(torch.from_numpy(pop).to(cuda), torch.from_numpy(cost).to(cuda), run)
    assert all(x.is_cuda for x in (res[0], res[1], res[3], res[4], res[5], res[6]))
    assert_same(tuple(x if isinstance(x, dict) else x.cpu().numpy() for x in res), one)


@pytest.mark.gpu
def test_evolutionary_optimizer_gpu_equals_cpu(cuda, task_domain):
    d = task_domain
    lb = float(d.cost_table.min(1).values.mean())
    kw = dict(islands=8, pool=10, select=3, iters=300)
    host = EvolutionaryOptimizer(d, use_kernel=True, **kw).run()
    dev = EvolutionaryOptimizer(d.to(cuda), **kw).run()
    assert dev.stats["engine"] == "eo_assign_kernel" and host.stats["engine"] == "eo_assign_twin"
    assert dev.best.is_cuda and torch.equal(dev.best.cpu(), host.best) and dev.best_cost == host.best_cost
    assert torch.equal(dev.costs.cpu(), host.costs) and torch.equal(dev.solutions.cpu(), host.solutions)
    assert dev.history == host.history
    assert {k: v for k, v in dev.stats.items() if k != "engine"} == {k: v for k, v in host.stats.items() if k != "engine"}
    print("kernel", dev.best_cost - lb)
    assert dev.best_cost <= lb + 3.0                                         # the quality bound, by the kernel
    small = random_assignment(8, 5, seed=1, density=0.3).to(cuda)
    assert "engine" not in EvolutionaryOptimizer(small, use_kernel=False, islands=2, pool=4, select=2, iters=3).run().stats


def _binding_args(cuda, L=8, V=5, I=4, P=6, iters=3):
    d = random_assignment(L, V, seed=1, density=0.3)
    if L <= 100:
        pop, cost = assign_start(d, I, P, 2)
    else:
        pop, cost = np.zeros((I, P, L), np.int16), np.zeros((I, P), np.float32)
    p = torch.from_numpy(pop).to(cuda)
    c = torch.from_numpy(cost).to(cuda)
    return {"cost": d.cost_table.to(cuda), "conflict": d.conflict.to(torch.uint8).to(cuda), "swap": True, "pop": p,
            "pop_cost": c, "born": torch.arange(P, dtype=torch.int32, device=cuda).repeat(I, 1),
            "best": p[:, 0].contiguous(), "best_cost": c[:, 0].contiguous(),
            "hist": torch.full((I, iters), -7.0, device=cuda), "iters": iters, "select": 3, "w": 0.7, "age_scale": 1.0,
            "seed": 1, "it_begin": 0, "island_base": 0, "stats": torch.zeros(4, dtype=torch.long, device=cuda)}


def _break(a, case, cuda):
    if case == "pop dtype":
        a["pop"] = a["pop"].int()
    elif case == "born dtype":
        a["born"] = a["born"].long()
    elif case == "cost dtype":
        a["cost"] = a["cost"].double()
    elif case == "pop shape":
        a["pop"] = a["pop"][:, :, :-1].contiguous()
    elif case == "best shape":
        a["best"] = a["best"][:-1].contiguous()
    elif case == "hist shape":
        a["hist"] = torch.full((4, 4), -7.0, device=cuda)
    elif case == "cpu tensor":
        a["pop_cost"] = a["pop_cost"].cpu()
    elif case == "P > 64":
        a["pop"] = torch.zeros((4, 65, 8), dtype=torch.int16, device=cuda)
        a["pop_cost"] = torch.zeros((4, 65), device=cuda)
        a["born"] = torch.arange(65, dtype=torch.int32, device=cuda).repeat(4, 1)
    elif case == "select > P":
        a["select"] = 7
    elif case == "value out of range":
        a["pop"][2, 3, 1] = 5
    elif case == "negative value":
        a["best"][1, 0] = -1
    elif case == "counter bound":
        a["it_begin"] = 2 ** 31 - 8                               # + 3 iterations + P 6 = 2^31 + 1
    elif case == "w > 1":
        a["w"] = 1.5
    elif case == "LDS":
        b = _binding_args(cuda, 600, 3, 2, 64)
        a.clear()
        a.update(b)
    else:
        raise KeyError(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["pop dtype", "born dtype", "cost dtype", "pop shape", "best shape", "hist shape",
                                  "cpu tensor", "P > 64", "select > P", "value out of range", "negative value",
                                  "counter bound", "w > 1", "LDS"])
def test_binding_validation(cuda, case):
    from avenir_amd import _native
    a = _binding_args(cuda)
    _break(a, case, cuda)
    with pytest.raises((RuntimeError, ValueError, TypeError)):
        _native.C().eo_assign(*a.values())
    torch.cuda.synchronize()
    assert (a["hist"] == -7.0).all() and int(a["stats"].sum()) == 0          # nothing was launched


@pytest.mark.gpu
def test_plan_queries_and_empty_runs(cuda):
    from avenir_amd import _native
    for P, L in ((10, 24), (64, 96), (5, 200), (64, 500), (64, 510), (2, 1), (33, 77)):
        assert tuple(_native.C().eo_assign_plan(P, L)) == E.eo_assign_plan(P, L)
    for P, M in ((5, 10), (64, 32), (10, 1), (64, 1), (33, 7)):
        assert tuple(_native.C().eo_meeting_plan(P, M)) == E.eo_meeting_plan(P, M)
    # no iterations, no islands: the state comes back as it went in
    d = random_assignment(8, 5, seed=1, density=0.3)
    pop, cost = assign_start(d, 4, 6, 2)
    out = eo_assign_advance(d.to(cuda), pop, cost, EoRun(0, 3), cuda)
    assert_same(out, eo_assign_reference(d, pop, cost, EoRun(0, 3)))
    out = eo_assign_advance(d.to(cuda), pop[:0], cost[:0], EoRun(3, 3), cuda)
    assert out[0].shape == (0, 8) and out[6].shape == (0, 3) and out[2] == {"inserted": 0, "stalls": 0, "improved": 0}
