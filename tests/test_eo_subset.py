"""Evolutionary-optimiser islands over feature subsets scored by naive Bayes (optimize/eo.py,
optimize/ga_subset.py): the twin's segments, global indexing, branches, invariants and edge shapes and
the dispatch of ``EvolutionaryOptimizer`` on the CPU; ``eo_subset_kernel`` bit-equal to the twin for every
split of the workgroup into islands and every row count, segmented launches, the class equal on both
devices and the binding's validation on the GPU."""
import functools

import numpy as np
import pytest
import torch

from avenir_amd.optimize import EoRun, EvolutionaryOptimizer, eo_subset_advance, eo_subset_reference
from avenir_amd.optimize.domains import FeatureSubsetDomain
from tests._eo import assert_same, check_invariants, segments


@functools.lru_cache(maxsize=None)
def _random(N, F, C, seed=0):
    """Random fp32 log-likelihoods whose labels follow the first features (so subsets differ in error)."""
    rng = np.random.default_rng(77 + 1000 * seed + 100 * F + C)
    LL = (-8.0 * rng.random((N, F, C))).astype(np.float32)
    prior = np.log(rng.dirichlet(np.full(C, 5.0))).astype(np.float32)
    labels = (LL[:, : max(1, F // 3), :].sum(1) + rng.normal(0, 2.0, (N, C))).argmax(1)
    labels[0] = C - 1
    return LL, prior, labels


def _domain(data, device="cpu", **kw):
    LL, prior, labels = data
    return FeatureSubsetDomain(LL.shape[1], loglik=torch.from_numpy(LL), log_prior=torch.from_numpy(prior),
                               labels=torch.from_numpy(labels), device=device, **kw)


_SHAPES = {  # N, F, C, min_size, max_size
    "reference": (517, 12, 3, 2, 8),
    "F1": (64, 1, 2, 0, 1),
    "F32-C16": (300, 32, 16, 1, 32),           # F C = 512: the tile is shorter than a wave
    "fixed_size": (517, 12, 3, 5, 5),          # every flip leaves the size range: every iteration stalls
    "N1": (1, 5, 2, 1, 5), "N63": (63, 5, 2, 1, 5), "N64": (64, 5, 2, 1, 5), "N65": (65, 5, 2, 1, 5),
    "N1000": (1000, 5, 2, 1, 5),
    "N2500": (2500, 5, 2, 1, 5),               # 1,024 threads, several tiles and a ragged last one
}


@functools.lru_cache(maxsize=None)
def _tables(shape):
    from avenir_amd.optimize.ga_subset import subset_tables
    N, F, C, lo, hi = _SHAPES[shape]
    d = _domain(_random(N, F, C), min_size=lo, max_size=hi)
    tb = subset_tables(d)
    assert tb is not None
    return d, tb


def _start(tb, n, P, seed, base=0):
    from avenir_amd.optimize.ga_subset import ga_subset_init, ga_subset_price, pack_masks
    pop = ga_subset_init(tb, n, P, seed, base)
    return pop, ga_subset_price(tb, pack_masks(pop))


def _price(tb):
    from avenir_amd.optimize.ga_subset import ga_subset_price, pack_masks
    return lambda s: ga_subset_price(tb, pack_masks(s))


@functools.lru_cache(maxsize=None)
def _branch_run():
    _, tb = _tables("reference")
    pop, cost = _start(tb, 8, 10, 7)
    trace = {}
    return tb, pop, cost, eo_subset_reference(tb, pop, cost, EoRun(300, 3, 0.7, 1.0, 7), trace=trace), trace


# ------------------------------------------------------------------------------------------- CPU
def test_twin_segments_equal_one_run_and_invariants_hold():
    tb, pop, cost, one, trace = _branch_run()
    twin = lambda *a, **k: eo_subset_advance(tb, *a[:3], "cpu", **k)
    cut = segments(twin, pop, cost, EoRun(300, 3, 0.7, 1.0, 7), 70, functools.partial(check_invariants, _price(tb), 10))
    assert_same(cut, one)
    check_invariants(_price(tb), 10, (pop, cost, None), one)
    st = one[2]
    print(st, "tied tournaments", trace["tied"])
    assert st["inserted"] > 0 and st["stalls"] > 0 and st["improved"] > 0 and trace["tied"] > 0
    assert st["inserted"] + st["stalls"] == 8 * 300
    assert one[0].dtype == np.int16 and one[3].dtype == np.int16 and ((one[3] == 0) | (one[3] == 1)).all()


def test_island_indexing_is_global():
    tb, pop, cost, full, _ = _branch_run()
    part_pop, part_cost = _start(tb, 5, 10, 7, 3)
    assert np.array_equal(part_pop, pop[3:]) and np.array_equal(part_cost, cost[3:])
    part = eo_subset_reference(tb, part_pop, part_cost, EoRun(300, 3, 0.7, 1.0, 7, 0, 3))
    for i in (0, 1, 3, 4, 5, 6):
        assert np.array_equal(full[i][3:], part[i]), i


def _edge(name):
    """(tables, pool, costs, EoRun) of an edge shape."""
    if name in ("F1", "F32-C16", "fixed_size"):
        _, tb = _tables(name)
        return (tb, *_start(tb, 5, 5, 2), EoRun(50, 3, 0.7, 1.0, 2))
    if name == "P2-select1":
        _, tb = _tables("reference")
        return (tb, *_start(tb, 5, 2, 2), EoRun(60, 1, 0.7, 1.0, 2))
    if name == "P64-select64":
        _, tb = _tables("reference")
        return (tb, *_start(tb, 3, 64, 2), EoRun(40, 64, 0.3, 1.0, 2))
    raise KeyError(name)


_EDGES = ("F1", "F32-C16", "fixed_size", "P2-select1", "P64-select64")


@pytest.mark.parametrize("name", _EDGES)
def test_edge_shapes(name):
    tb, pop, cost, run = _edge(name)
    one = eo_subset_reference(tb, pop, cost, run)
    check_invariants(_price(tb), pop.shape[1], (pop, cost, None), one)
    assert_same(segments(functools.partial(eo_subset_reference, tb), pop, cost, run, 17), one)
    if name == "fixed_size":
        assert one[2] == {"inserted": 0, "stalls": 5 * 50, "improved": 0} and np.array_equal(one[3], pop)
    else:
        assert one[2]["inserted"] > 0


def test_dispatch_on_the_cpu():
    from avenir_amd.optimize import ga_subset as gs
    d, tb = _tables("reference")
    kw = dict(islands=4, pool=5, select=3, iters=30, seed=1)
    assert EvolutionaryOptimizer(d, **kw)._island_engine() is None
    assert "engine" not in EvolutionaryOptimizer(d, **kw).run().stats
    res = EvolutionaryOptimizer(d, use_kernel=True, **kw).run()
    assert res.stats["engine"] == "eo_subset_host" and res.stats["inserted"] + res.stats["stalls"] == 4 * 30
    assert res.costs.shape == (4,) and res.solutions.shape == (4, 12) and len(res.history) == 30
    assert float(d.cost(res.best.view(1, -1))[0]) == pytest.approx(res.best_cost, rel=1e-5)
    # tied groups and a cost callback: the torch path even when asked for the kernel
    grouped = _domain(_random(517, 12, 3), min_size=2, max_size=8, groups=[[0, 1]])
    assert EvolutionaryOptimizer(grouped, use_kernel=True, **kw)._island_engine() is None
    fn = FeatureSubsetDomain(12, cost_fn=lambda s: s.float().sum(1))
    assert EvolutionaryOptimizer(fn, use_kernel=True, **kw)._island_engine() is None
    assert gs.EO_ROW_CAP <= gs.SA_ROW_CAP


# ------------------------------------------------------------------------------------------- GPU
def _case(name):
    if name in _EDGES:
        return (*_edge(name), 0)
    if name.startswith("N"):                    # row counts: one partial group, full groups, several tiles
        shape, w = name.split("-w")
        _, tb = _tables(shape)
        return (tb, *_start(tb, 5, 5, 3), EoRun(40, 3, 0.7, 1.0, 3), int(w))
    if name.startswith("islands-"):
        _, tb = _tables("reference")
        return (tb, *_start(tb, int(name.split("-")[1]), 5, 7), EoRun(60, 3, 0.7, 1.0, 7), 0)
    if name == "island-base":
        _, tb = _tables("reference")
        return (tb, *_start(tb, 5, 10, 7, 3), EoRun(300, 3, 0.7, 1.0, 7, 0, 3), 0)
    raise KeyError(name)


_CASES = _EDGES + tuple(f"{n}-w{w}" for n in ("N1", "N63", "N64", "N65", "N1000", "N2500") for w in (1, 2, 16)) + (
    "islands-1", "islands-63", "islands-65", "islands-130", "island-base")


@pytest.mark.gpu
@pytest.mark.parametrize("name", _CASES)
def test_kernel_bit_equal_to_twin(cuda, name):
    tb, pop, cost, run, w = _case(name)
    want = eo_subset_reference(tb, pop, cost, run)
    got = eo_subset_advance(tb, pop, cost, run, cuda, waves_per_island=w)
    assert_same(got, want)
    if name == "islands-130":
        assert min(want[2].values()) > 0
    if name == "island-base":
        full = _branch_run()[3]
        for i in (0, 1, 3, 4, 5, 6):
            assert np.array_equal(full[i][3:], got[i]), i


@pytest.mark.gpu
def test_segmented_launches_equal_one_launch_and_the_twin(cuda):
    _, tb = _tables("reference")
    pop, cost = _start(tb, 20, 5, 7)
    kernel = lambda p, c, run, **st: eo_subset_advance(tb, p, c, run, cuda, **st)
    run = EoRun(100, 3, 0.7, 1.0, 7)
    one = kernel(pop, cost, run)
    assert_same(segments(kernel, pop, cost, run, 40), one)
    assert_same(one, eo_subset_reference(tb, pop, cost, run))


@pytest.mark.gpu
def test_evolutionary_optimizer_gpu_equals_cpu(cuda):
    kw = dict(islands=20, pool=5, select=3, iters=80, seed=9)
    data = _random(517, 12, 3)
    host = EvolutionaryOptimizer(_domain(data, min_size=2, max_size=8), use_kernel=True, **kw).run()
    dev = EvolutionaryOptimizer(_domain(data, device="cuda", min_size=2, max_size=8), **kw).run()
    assert dev.stats["engine"] == "eo_subset_kernel" and host.stats["engine"] == "eo_subset_host"
    assert dev.best_cost == host.best_cost and torch.equal(dev.best.cpu(), host.best)
    assert torch.equal(dev.costs.cpu(), host.costs) and torch.equal(dev.solutions.cpu(), host.solutions)
    assert dev.history == host.history
    assert {k: v for k, v in dev.stats.items() if k != "engine"} == {k: v for k, v in host.stats.items() if k != "engine"}


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["pop dtype", "pop shape", "cpu tensor", "select > P", "mask value", "counter bound",
                                  "waves"])
def test_binding_validation(cuda, case):
    from avenir_amd import _native
    from avenir_amd.optimize.ga_subset import _device_tables
    _, tb = _tables("reference")
    pop, cost = _start(tb, 4, 6, 2)
    p, c = torch.from_numpy(pop).to(cuda), torch.from_numpy(cost).to(cuda)
    a = {"min": tb["min_size"], "max": tb["max_size"], "pop": p, "pop_cost": c,
         "born": torch.arange(6, dtype=torch.int32, device=cuda).repeat(4, 1),
         "best": p[:, 0].contiguous(), "best_cost": c[:, 0].contiguous(), "hist": torch.full((4, 3), -7.0, device=cuda),
         "iters": 3, "select": 3, "w": 0.7, "age_scale": 1.0, "seed": 1, "it_begin": 0, "island_base": 0,
         "stats": torch.zeros(4, dtype=torch.long, device=cuda), "waves": 0}
    if case == "pop dtype":
        a["pop"] = a["pop"].int()
    elif case == "pop shape":
        a["pop"] = a["pop"][:, :, :-1].contiguous()
    elif case == "cpu tensor":
        a["best_cost"] = a["best_cost"].cpu()
    elif case == "select > P":
        a["select"] = 7
    elif case == "mask value":
        a["pop"][1, 2, 0] = 2
    elif case == "counter bound":
        a["it_begin"] = 2 ** 31 - 8
    elif case == "waves":
        a["waves"] = 3
    with pytest.raises((RuntimeError, ValueError, TypeError)):
        _native.C().eo_subset(*_device_tables(tb, cuda), *a.values())
    torch.cuda.synchronize()
    assert (a["hist"] == -7.0).all() and int(a["stats"].sum()) == 0          # nothing was launched
