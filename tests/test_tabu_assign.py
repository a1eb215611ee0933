"""Tabu search over assignment domains (optimize/tabu.py): the numpy twin against the generic torch
path of ``TabuSearch`` (exact), segments, the branches by the twin's own counters, invariants, the
dispatch and the world size on the CPU; ``tabu_assign_kernel`` against the twin (exact in every
output), segmented launches, the class on both devices and the binding's validation on the GPU."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from avenir_amd.optimize import AssignmentDomain, TabuRun, TabuSearch, tabu_assign_advance, tabu_assign_reference
from avenir_amd.optimize import tabu as T
from avenir_amd.optimize.sa import sa_assign_init
from tests._dist import run_world


def _random_assignment(L=24, V=10, seed=0, density=0.15):
    g = torch.Generator().manual_seed(seed)
    cost = torch.rand((L, V), generator=g) * 100
    conf = torch.rand((L, L), generator=g) < density
    conf = conf | conf.T
    return AssignmentDomain(cost, conf, invalid_cost=1e3)


def _integer_table(d):
    """The same domain with the table ``floor(cost / 25)``: four cost levels, so minima tie."""
    return AssignmentDomain(torch.floor(d.cost_table / 25), d.conflict, invalid_cost=d.invalid_cost)


def _plain(L, V, seed=1):
    g = torch.Generator().manual_seed(seed)
    return AssignmentDomain(torch.rand((L, V), generator=g) * 100, None, invalid_cost=1e3)


def _start(d, P, seed=2, base=0, total=None):
    sol = sa_assign_init(d, P, seed, base, total=total)
    return sol.numpy(), d.evaluate(sol).numpy()


def _raw_start(d, P, seed=2):
    """Uniform values with no regard for conflicts: many starts are invalid and priced ``invalid_cost``."""
    g = torch.Generator().manual_seed(seed)
    sol = torch.randint(0, d.V, (P, d.L), generator=g)
    return sol.numpy(), d.evaluate(sol).numpy()


def _twin(d, sol, cost, run, **state):
    conf = None if d.conflict is None else d.conflict.numpy()
    return tabu_assign_reference(d.cost_table.numpy(), conf, sol, cost, run, **state)


_NAMES = ("best", "best_cost", "stats", "sol", "cost", "tabu", "hist")


def _assert_same(a, b):
    for name, x, y in zip(_NAMES, a, b):
        if name == "stats":
            assert x == y, (x, y)
        else:
            x, y = np.asarray(x), np.asarray(y)
            assert x.shape == y.shape, name
            if x.dtype.kind == "f":        # the same bits; NaN never appears with finite tables
                assert np.array_equal(x.astype(np.float32).view(np.uint32), y.astype(np.float32).view(np.uint32)), name
            else:
                assert np.array_equal(x, y), name


def _segments(advance, sol, cost, cuts, tenure):
    """The run cut at ``cuts`` through the returned state -> the outputs of one run."""
    state = {}
    stats = {"moves": 0, "stalls": 0, "aspirated": 0}
    hists, b = [], 0
    for n in cuts:
        best, bc, st, sol, cost, tabu, h = advance(sol, cost, TabuRun(n, tenure, b), **state)
        state = {"tabu": tabu, "best": best, "best_cost": bc}
        hists.append(np.asarray(h))
        for k in stats:
            stats[k] += st[k]
        b += n
    return best, bc, stats, sol, cost, tabu, np.concatenate(hists, 1)


# ---- CPU ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,V,density", [(24, 10, 0.15), (65, 7, 0.1), (12, 70, 0.3), (5, 3, 0.6), (3, 2, 1.0)])
def test_twin_equals_generic_path(L, V, density):
    d = _random_assignment(L, V, seed=1, density=density)
    P, iters, tenure, seed = 6, 40, 5, 3
    res = TabuSearch(d, n_chains=P, iters=iters, tenure=tenure, seed=seed).run()
    assert "engine" not in res.stats
    sol, cost = _start(d, P, seed, 0, total=P)
    best, bc, _, _, _, _, hist = _twin(d, sol, cost, TabuRun(iters, tenure))
    assert np.array_equal(bc.view(np.uint32), res.costs.numpy().view(np.uint32))
    assert np.array_equal(best, res.solutions.numpy())
    assert hist.min(0).tolist() == res.history


def test_twin_segments_equal_one_run():
    d = _random_assignment(8, 5, seed=1, density=0.3)
    sol, cost = _start(d, 40)
    whole = _twin(d, sol, cost, TabuRun(50, 4))
    cut = _segments(functools.partial(_twin, d), sol, cost, (7, 20, 1, 22), 4)
    _assert_same(cut, whole)
    assert whole[2]["aspirated"] > 0 and (whole[5] >= 0).any()      # the table matters across the cuts


def _count_ties(d, sol, cost, iters, tenure):
    """Iterations (over all chains) whose smallest admissible price is held by two cells or more:
    the twin advanced one iteration at a time, the neighbourhood scored here by the steps of the
    module docstring on the state before each."""
    C, conf = d.cost_table.numpy(), d.conflict.numpy()
    L, V = C.shape
    state, ties = {}, 0
    bc = cost.copy()
    tabu = np.full((sol.shape[0], L, V), -1, np.int32)
    for it in range(iters):
        for p in range(sol.shape[0]):
            cur = C[np.arange(L), sol[p]]
            nc = np.float32(cost[p]) + ((C - cur[:, None]).astype(np.float32) / np.float32(L)).astype(np.float32)
            occ = sol[p][:, None] == np.arange(V)[None, :]
            bad = occ | ((conf.astype(np.int32) @ occ.astype(np.int32)) > 0)
            adm = ~bad & ((tabu[p] <= it) | (nc < bc[p]))
            if adm.any():
                ties += int((nc[adm] == nc[adm].min()).sum() > 1)
        best, bc, _, sol, cost, tabu, _ = _twin(d, sol, cost, TabuRun(1, tenure, it), **state)
        state = {"tabu": tabu, "best": best, "best_cost": bc}
    return ties


def test_every_branch_is_taken():
    # the tabu table changes the choice, and aspiration overrides it
    d = _random_assignment(8, 5, seed=1, density=0.3)
    sol, cost = _start(d, 300)
    with_tabu = _twin(d, sol, cost, TabuRun(50, 4))
    assert with_tabu[2]["aspirated"] > 0 and with_tabu[2]["moves"] > 0
    assert not np.array_equal(with_tabu[3], _twin(d, sol, cost, TabuRun(50, 0))[3])
    # ties on nearly every move go to the smallest flat index
    d = _integer_table(_random_assignment(7, 4, seed=1, density=0.3))
    sol, cost = _start(d, 64)
    assert _count_ties(d, sol, cost, 60, 3) > 0
    # a neighbourhood exhausted by a long tenure stalls (starts without conflicts are valid)
    d = _plain(3, 3)
    sol, cost = _start(d, 16)
    st = _twin(d, sol, cost, TabuRun(40, 100))[2]
    assert st["stalls"] > 0 and st["moves"] > 0 and st["moves"] + st["stalls"] == 16 * 40
    # tenure 0 never masks a cell: nothing is ever aspirated, nothing stalls
    d = _random_assignment(6, 4, seed=1, density=0.3)
    sol, cost = _start(d, 32)
    st = _twin(d, sol, cost, TabuRun(30, 0))[2]
    assert st["aspirated"] == 0 and st["moves"] > 0
    # one value: no cell is a move
    d = _plain(4, 1)
    sol, cost = _start(d, 4)
    out = _twin(d, sol, cost, TabuRun(5, 2))
    assert out[2] == {"moves": 0, "stalls": 20, "aspirated": 0} and np.array_equal(out[3], sol)
    # one position
    d = _random_assignment(1, 5, seed=1, density=0.3)
    sol, cost = _start(d, 4)
    out = _twin(d, sol, cost, TabuRun(10, 2))
    assert out[2]["moves"] > 0 and np.abs(out[1] - d.cost_table.numpy().min()).max() <= 1e-4
    # no conflict table
    d = _plain(6, 4)
    sol, cost = _start(d, 8)
    assert _twin(d, sol, cost, TabuRun(20, 3))[2]["moves"] == 8 * 20


def test_infinite_table_entry_is_never_taken():
    d = _plain(6, 6)
    sol, cost = _start(d, 3)
    C = d.cost_table.clone()
    for l in range(6):      # per position a value that no start holds, and the cheapest of the rest
        free = [v for v in range(6) if v not in sol[:, l].tolist()]
        C[l, free[0]] = float("inf")
    C[0, [v for v in range(6) if torch.isfinite(C[0, v])][0]] = -5.0
    d = AssignmentDomain(C, None, invalid_cost=1e3)
    cost = d.evaluate(torch.from_numpy(sol)).numpy()
    best, bc, st, s, c, _, hist = _twin(d, sol, cost, TabuRun(60, 2))
    assert st["moves"] > 0 and np.isfinite(hist).all() and np.isfinite(c).all()
    for x in (best, s):
        assert torch.isfinite(C[torch.arange(6), torch.from_numpy(x)]).all()


def test_invariants():
    d = _random_assignment(24, 10, seed=1, density=0.15)
    gen = torch.Generator().manual_seed(4)
    sol, ok = d.random(16, gen)
    assert ok.all()
    cost = d.evaluate(sol)
    best, bc, _, s, c, _, hist = _twin(d, sol.numpy(), cost.numpy(), TabuRun(100, 7))
    assert d.valid(torch.from_numpy(best)).all() and d.valid(torch.from_numpy(s)).all()
    assert (np.diff(hist, axis=1) <= 0).all() and (hist[:, 0] <= cost.numpy()).all()
    assert np.array_equal(hist[:, -1], bc)
    assert np.abs(d.cost(torch.from_numpy(s)).numpy() - c).max() <= 1e-3
    assert np.abs(d.cost(torch.from_numpy(best)).numpy() - bc).max() <= 1e-3


def test_dispatch_on_the_cpu():
    d = _random_assignment(8, 5, seed=1, density=0.3)
    kw = dict(n_chains=4, iters=10, tenure=3, seed=1)
    assert "engine" not in TabuSearch(d, **kw).run().stats
    assert "engine" not in TabuSearch(d, use_kernel=False, **kw).run().stats
    res = TabuSearch(d, use_kernel=True, **kw).run()
    assert res.stats["engine"] == "tabu_assign_twin"
    assert res.stats["moves"] + res.stats["stalls"] == 4 * 10 and "aspirated" in res.stats
    big = _random_assignment(200, 100, seed=1, density=0.01)
    assert T.tabu_assign_lds(200, 100) > T.LDS_LIMIT
    assert "engine" not in TabuSearch(big, n_chains=2, iters=2, tenure=3, seed=1, use_kernel=True).run().stats


def test_lds_plan():
    assert T.tabu_assign_plan(24, 10) == (4, True, 4 * (960 + 96 + 480 + 48) + 960 + 576)
    assert T.tabu_assign_plan(20, 130)[:2] == (2, True)
    assert T.tabu_assign_plan(240, 8)[:2] == (1, False)      # the tables stay in global memory
    for L, V in ((24, 10), (20, 130), (240, 8), (65, 7), (1, 5), (4, 1)):
        assert T.tabu_assign_lds(L, V) <= T.LDS_LIMIT


def _tabu_world(rank, world, n):
    from avenir_amd.parallel.comm import get_comm
    d = _random_assignment(8, 5, seed=1, density=0.3)
    r = TabuSearch(d, n_chains=n, iters=30, tenure=4, seed=5, comm=get_comm(), use_kernel=True).run()
    return r.best.numpy(), r.best_cost, r.costs.numpy(), r.history, r.stats


def test_two_ranks_equal_one_process():
    got = run_world(_tabu_world, 2, 4)
    d = _random_assignment(8, 5, seed=1, density=0.3)
    one = TabuSearch(d, n_chains=8, iters=30, tenure=4, seed=5, use_kernel=True).run()
    assert np.array_equal(np.concatenate([g[2] for g in got]), one.costs.numpy())
    for best, best_cost, _, history, stats in got:
        assert np.array_equal(best, one.best.numpy()) and best_cost == one.best_cost
        assert history == one.history and stats == one.stats


# ---- GPU ---------------------------------------------------------------------------------------
def _case(name):
    """(domain, start solutions, start costs, TabuRun) of a kernel case."""
    if name == "24x10x16":          # lanes idle in the last cell step
        d = _random_assignment(24, 10, seed=1, density=0.15)
        return (d, *_start(d, 16), TabuRun(60, 7))
    if name == "65x7x8-invalid":    # L above a wave; invalid starts priced at invalid_cost
        d = _random_assignment(65, 7, seed=1, density=0.1)
        sol, cost = _raw_start(d, 8)
        assert (cost == np.float32(d.invalid_cost)).any()
        return d, sol, cost, TabuRun(60, 7)
    if name == "20x130x4-ties":     # V above a wave, ties across lanes, two chains per workgroup
        d = _integer_table(_random_assignment(20, 130, seed=1, density=0.3))
        return (d, *_start(d, 4), TabuRun(40, 5))
    if name == "8x5x300":           # several workgroups
        d = _random_assignment(8, 5, seed=1, density=0.3)
        return (d, *_start(d, 300), TabuRun(50, 4))
    if name == "8x5x302":           # and a partial last one (two idle waves)
        d = _random_assignment(8, 5, seed=1, density=0.3)
        return (d, *_start(d, 302), TabuRun(50, 4))
    if name == "3x3x16-stalls":
        d = _plain(3, 3)
        return (d, *_start(d, 16), TabuRun(40, 100))
    if name == "4x1":
        d = _plain(4, 1)
        return (d, *_start(d, 4), TabuRun(5, 2))
    if name == "1x5":
        d = _random_assignment(1, 5, seed=1, density=0.3)
        return (d, *_start(d, 4), TabuRun(10, 2))
    if name == "no-conflict":
        d = _plain(6, 4)
        return (d, *_start(d, 8), TabuRun(20, 3))
    if name == "chain-base":
        d = _random_assignment(8, 5, seed=1, density=0.3)
        return (d, *_start(d, 5, base=11, total=20), TabuRun(30, 4, 0, 11))
    if name == "240x8x3-global":    # the tables do not fit beside the chain: read from global memory
        d = _random_assignment(240, 8, seed=1, density=0.02)
        return (d, *_raw_start(d, 3), TabuRun(25, 6))
    if name == "last-iteration":    # it_begin + iters + tenure = 2^31 - 1
        d = _random_assignment(8, 5, seed=1, density=0.3)
        return (d, *_start(d, 4), TabuRun(2, 7, 2 ** 31 - 10))
    raise KeyError(name)


_CASES = ("24x10x16", "65x7x8-invalid", "20x130x4-ties", "8x5x300", "8x5x302", "3x3x16-stalls", "4x1", "1x5",
          "no-conflict", "chain-base", "240x8x3-global", "last-iteration")


@pytest.mark.gpu
@pytest.mark.parametrize("name", _CASES)
def test_kernel_bit_equal_to_twin(cuda, name):
    d, sol, cost, run = _case(name)
    want = _twin(d, sol, cost, run)
    got = tabu_assign_advance(d.to(cuda), sol, cost, run, cuda)
    _assert_same(got, want)
    if name == "3x3x16-stalls":
        assert want[2]["stalls"] > 0
    if name == "8x5x300":
        assert want[2]["aspirated"] > 0


@pytest.mark.gpu
def test_segmented_launches_equal_one_launch_and_the_twin(cuda):
    d = _random_assignment(8, 5, seed=1, density=0.3)
    sol, cost = _start(d, 40)
    dc = d.to(cuda)
    kernel = lambda s, c, run, **st: tabu_assign_advance(dc, s, c, run, cuda, **st)
    one = kernel(sol, cost, TabuRun(50, 4))
    cut = _segments(kernel, sol, cost, (7, 20, 1, 22), 4)
    _assert_same(cut, one)
    _assert_same(one, _twin(d, sol, cost, TabuRun(50, 4)))
    # resident state: tensors on the GPU in, tensors on the GPU out
    res = kernel(torch.from_numpy(sol).to(cuda), torch.from_numpy(cost).to(cuda), TabuRun(50, 4))
    assert all(x.is_cuda for x in (res[0], res[1], res[3], res[4], res[5], res[6]))
    _assert_same(tuple(x if isinstance(x, dict) else x.cpu().numpy() for x in res), one)


@pytest.mark.gpu
def test_tabu_search_gpu_equals_cpu(cuda):
    d = _random_assignment(24, 10, seed=1, density=0.15)
    kw = dict(n_chains=16, iters=60, tenure=7, seed=3)
    host = TabuSearch(d, use_kernel=True, **kw).run()
    dev = TabuSearch(d.to(cuda), **kw).run()
    assert dev.stats["engine"] == "tabu_assign_kernel" and host.stats["engine"] == "tabu_assign_twin"
    assert dev.best.is_cuda and torch.equal(dev.best.cpu(), host.best) and dev.best_cost == host.best_cost
    assert torch.equal(dev.costs.cpu(), host.costs) and torch.equal(dev.solutions.cpu(), host.solutions)
    assert dev.history == host.history
    assert {k: v for k, v in dev.stats.items() if k != "engine"} == {k: v for k, v in host.stats.items() if k != "engine"}
    assert "engine" not in TabuSearch(d.to(cuda), use_kernel=False, n_chains=4, iters=3, tenure=2, seed=3).run().stats


def _binding_args(cuda, L=8, V=5, P=4, iters=3):
    d = _random_assignment(L, V, seed=1, density=0.3)
    sol, cost = _start(d, P)
    s = torch.from_numpy(sol).to(torch.int16).to(cuda)
    c = torch.from_numpy(cost).to(cuda)
    return {"cost": d.cost_table.to(cuda), "conflict": d.conflict.to(torch.uint8).to(cuda), "sol": s, "cur_cost": c,
            "best_sol": s.clone(), "best_cost": c.clone(),
            "tabu": torch.full((P, L, V), -1, dtype=torch.int32, device=cuda),
            "hist": torch.full((P, iters), -7.0, device=cuda), "iters": iters, "tenure": 2, "it_begin": 0,
            "stats": torch.zeros(4, dtype=torch.long, device=cuda)}


def _break(a, case, cuda):
    if case == "sol dtype":
        a["sol"] = a["sol"].int()
    elif case == "tabu dtype":
        a["tabu"] = a["tabu"].long()
    elif case == "cost dtype":
        a["cost"] = a["cost"].double()
    elif case == "tabu shape":
        a["tabu"] = a["tabu"][:, :, :-1].contiguous()
    elif case == "hist shape":
        a["hist"] = torch.zeros((4, 4), device=cuda)
    elif case == "cpu tensor":
        a["cur_cost"] = a["cur_cost"].cpu()
    elif case == "stats size":
        a["stats"] = torch.zeros(3, dtype=torch.long, device=cuda)
    elif case == "iteration range":
        a["it_begin"], a["tenure"] = 2 ** 31 - 5, 2             # + 3 iterations = 2^31
    elif case == "negative tenure":
        a["tenure"] = -1
    elif case == "V = 40000":
        a["cost"] = torch.zeros((8, 40000), device=cuda)
        a["tabu"] = torch.full((4, 8, 40000), -1, dtype=torch.int32, device=cuda)
    elif case == "LDS":
        b = _binding_args(cuda, 200, 100, 2)
        a.clear()
        a.update(b)
    else:
        raise KeyError(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["sol dtype", "tabu dtype", "cost dtype", "tabu shape", "hist shape", "cpu tensor",
                                  "stats size", "iteration range", "negative tenure", "V = 40000", "LDS"])
def test_binding_validation(cuda, case):
    from avenir_amd import _native
    a = _binding_args(cuda)
    _break(a, case, cuda)
    with pytest.raises((RuntimeError, ValueError)):
        _native.C().tabu_assign(*a.values())
    torch.cuda.synchronize()
    assert (a["hist"] == a["hist"].flatten()[0]).all() and int(a["stats"].sum()) == 0      # nothing was launched


@pytest.mark.gpu
def test_launcher_checks_and_empty_runs(cuda):
    from avenir_amd import _native
    for L, V in ((24, 10), (20, 130), (240, 8), (200, 100), (1, 1), (65, 7)):
        assert _native.C().tabu_assign_lds(L, V) == T.tabu_assign_lds(L, V)
    d = _random_assignment(8, 5, seed=1, density=0.3)
    sol, cost = _start(d, 4)
    bad = sol.copy()
    bad[2, 3] = d.V
    with pytest.raises(ValueError):
        tabu_assign_advance(d.to(cuda), bad, cost, TabuRun(3, 2), cuda)
    bad[2, 3] = -1
    with pytest.raises(ValueError):
        tabu_assign_advance(d.to(cuda), bad, cost, TabuRun(3, 2), cuda)
    # no iterations, no chains: the state comes back as it went in
    out = tabu_assign_advance(d.to(cuda), sol, cost, TabuRun(0, 2), cuda)
    _assert_same(out, _twin(d, sol, cost, TabuRun(0, 2)))
    out = tabu_assign_advance(d.to(cuda), sol[:0], cost[:0], TabuRun(3, 2), cuda)
    assert out[0].shape == (0, 8) and out[6].shape == (0, 3) and out[2] == {"moves": 0, "stalls": 0, "aspirated": 0}
