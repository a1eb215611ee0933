"""The island GA over a meeting-schedule domain as one K22 launch
(csrc/kernels/optim.hip::ga_meeting_kernel) and its numpy twin (optimize/ga_meeting.py): the twin's
validity and price against MeetingScheduleDomain, chunked runs and island indexing, edge shapes,
dispatch in GeneticAlgorithm; on the GPU the kernel bit-equal to the twin, the class equal on both
devices, and the binding's validation."""
import functools

import numpy as np
import pytest
import torch

from avenir_amd.optimize.domains import MeetingScheduleDomain


@functools.lru_cache(maxsize=None)
def _instance(M, Q, seed):
    from avenir_amd.optimize.ga_meeting import meeting_tables
    d = MeetingScheduleDomain.random_instance(M, Q, seed=seed)
    return d, meeting_tables(d)


def _start(tb, I, P, seed, base):
    from avenir_amd.optimize.ga_meeting import ga_meeting_init, ga_meeting_price
    pop = ga_meeting_init(tb, I, P, seed, base)
    return pop, ga_meeting_price(tb, pop)


def _in_range(tb, pop):
    return bool((pop >= 0).all() and (pop < tb["cards"]).all())


# seeds chosen so that each sample of 512 random schedules holds valid and invalid rows
# (random (32, 64) schedules are valid at a rate of about 1 %)
@pytest.mark.parametrize("M,Q,seed", [(1, 3, 0), (2, 4, 0), (10, 20, 3), (32, 64, 2)])
def test_price_and_validity_match_domain(M, Q, seed):
    from avenir_amd.optimize.ga_meeting import ga_meeting_price, ga_meeting_valid
    d, tb = _instance(M, Q, seed)
    assert tb is not None
    g = torch.Generator().manual_seed(100 + seed)
    sol = torch.stack([torch.randint(0, int(c), (512,), generator=g) for c in d.cards], 1)
    want = d.valid(sol).numpy()
    got = ga_meeting_valid(tb, sol.numpy())
    assert got.dtype == np.bool_ and np.array_equal(got, want)
    if M >= 2:
        assert want.any() and not want.all()
    price = ga_meeting_price(tb, sol.numpy())
    assert price.dtype == np.float32 and np.isinf(price[~want]).all()
    ref = d.cost(sol).numpy()[want]
    rel = np.abs(price[want] - ref) / np.abs(ref)
    print(f"M={M} Q={Q}: {int(want.sum())} valid, max relative difference {rel.max(initial=0.0):.3g}")
    assert (rel <= 1e-5).all()


def test_twin_chunks_equal_one_run():
    from avenir_amd.optimize.ga_meeting import ga_meeting_reference
    _, tb = _instance(10, 20, 3)
    pop, pc = _start(tb, 5, 16, 7, 11)
    one = ga_meeting_reference(tb, pop, pc, 12, 6, 5, True, True, 7, 11)
    a = ga_meeting_reference(tb, pop, pc, 5, 6, 5, True, True, 7, 11)
    b = ga_meeting_reference(tb, a[0], a[1], 7, 6, 5, True, True, 7, 11, gen_base=5)
    assert np.array_equal(one[0], b[0]) and np.array_equal(one[1], b[1])
    assert np.array_equal(one[2], np.concatenate([a[2], b[2]], 1))
    assert one[0].dtype == np.int16 and one[1].dtype == np.float32 and one[2].dtype == np.float32
    assert (np.diff(one[2], axis=1) <= 0).all()                     # elitism: the best never gets worse
    assert np.isfinite(one[2][:, -1]).all()


def test_island_indexing_is_global():
    """Islands [3, 8) run alone equal rows 3..7 of islands [0, 8): world-size invariance."""
    from avenir_amd.optimize.ga_meeting import ga_meeting_reference
    _, tb = _instance(10, 20, 3)
    pop, pc = _start(tb, 8, 12, 21, 0)
    part_pop, part_pc = _start(tb, 5, 12, 21, 3)
    assert np.array_equal(part_pop, pop[3:]) and np.array_equal(part_pc, pc[3:])
    full = ga_meeting_reference(tb, pop, pc, 6, 5, 4, False, True, 21, 0)
    part = ga_meeting_reference(tb, part_pop, part_pc, 6, 5, 4, False, True, 21, 3)
    for f, p in zip(full, part):
        assert np.array_equal(f[3:], p)


@pytest.mark.parametrize("case", ["M1", "P2", "P64_purge", "P_plus_r_64", "one_minute"])
def test_twin_edge_shapes(case):
    from avenir_amd.optimize.ga_meeting import ga_meeting_reference, meeting_tables
    M, Q, P, m, r, purge = {"M1": (1, 3, 6, 3, 2, True), "P2": (5, 10, 2, 1, 1, True),
                            "P64_purge": (5, 10, 64, 20, 32, True), "P_plus_r_64": (5, 10, 40, 12, 24, False),
                            "one_minute": (5, 10, 12, 6, 4, False)}[case]
    if case == "one_minute":
        src = MeetingScheduleDomain.random_instance(M, Q, seed=0)
        parts = [src.member[:, i].nonzero().view(-1).tolist() for i in range(M)]
        d = MeetingScheduleDomain(parts, (src.dur / 60).tolist(), Q, src.ordered, src.blocked, src.role_w.tolist(),
                                  minutes=(0,))
        tb = meeting_tables(d)
        assert tb["cards"][2] == 1
    else:
        _, tb = _instance(M, Q, 0)
    pop, pc = _start(tb, 3, P, 4, 0)
    out, oc, hist = ga_meeting_reference(tb, pop, pc, 6, m, r, purge, True, 4, 0)
    assert out.shape == pop.shape and oc.shape == pc.shape and hist.shape == (3, 6)
    assert _in_range(tb, pop) and _in_range(tb, out)
    if case == "one_minute":
        assert (out[..., 2::3] == 0).all()
    if purge:
        assert (np.diff(hist, axis=1) <= 0).all()


def test_dispatch_on_the_cpu():
    from avenir_amd.optimize.search import GeneticAlgorithm
    from avenir_amd.utils.resilience import RecoveryConfig
    d, _ = _instance(6, 10, 1)
    kw = dict(islands=2, pool=12, mating=5, replacement=4, generations=6, seed=5)
    twin = GeneticAlgorithm(d, use_kernel=True, **kw).run()
    assert twin.stats.get("engine") == "ga_meeting_twin"
    assert len(twin.history) == 6 and np.isfinite(twin.best_cost)
    assert bool(d.valid(twin.best.view(1, -1))[0])
    assert float(d.cost(twin.best.view(1, -1))[0]) == pytest.approx(float(twin.best_cost), rel=1e-5)
    default = GeneticAlgorithm(d, **kw).run()
    generic = GeneticAlgorithm(d, use_kernel=False, **kw).run()
    assert "engine" not in (default.stats or {}) and "engine" not in (generic.stats or {})
    assert torch.equal(default.best, generic.best) and default.best_cost == generic.best_cost
    assert default.history == generic.history
    # outside the kernel's limits, or with checkpointing: the generic path even when asked for the kernel
    big = MeetingScheduleDomain.random_instance(33, 40, seed=0)
    assert GeneticAlgorithm(big, use_kernel=True, **kw)._island_engine() is None
    assert "engine" not in (GeneticAlgorithm(big, use_kernel=True, **dict(kw, generations=1)).run().stats or {})
    assert GeneticAlgorithm(d, use_kernel=True, recovery=RecoveryConfig(), **kw)._island_engine() is None


# ------------------------------------------------------------------------------------------- GPU
_SHAPES = {  # M, Q, domain seed, P, m, r, G
    "reference": (10, 20, 3, 30, 10, 10, 30),
    "smallest": (1, 3, 0, 2, 1, 1, 5),
    "largest": (32, 64, 2, 64, 20, 32, 4),
}


@functools.lru_cache(maxsize=None)
def _twin_run(shape, islands, purge_first, mutate):
    from avenir_amd.optimize.ga_meeting import ga_meeting_reference
    M, Q, dseed, P, m, r, G = _SHAPES[shape]
    _, tb = _instance(M, Q, dseed)
    pop, pc = _start(tb, islands, P, 5, 100)
    return pop, pc, ga_meeting_reference(tb, pop, pc, G, m, r, purge_first, mutate, 5, 100)


def _assert_bit_equal(want, got):
    for w, g_ in zip(want, got):
        assert w.dtype == g_.dtype and np.array_equal(w, g_)


@pytest.mark.gpu
@pytest.mark.parametrize("islands", [1, 256])
@pytest.mark.parametrize("purge_first,mutate", [(True, True), (False, True), (True, False)])
def test_kernel_bit_equal_to_twin(cuda, islands, purge_first, mutate):
    from avenir_amd.optimize.ga_meeting import ga_meeting_run
    M, Q, dseed, P, m, r, G = _SHAPES["reference"]
    _, tb = _instance(M, Q, dseed)
    pop, pc, want = _twin_run("reference", islands, purge_first, mutate)
    got = ga_meeting_run(tb, pop, pc, G, m, r, purge_first, mutate, 5, 100, torch.device("cuda"))
    _assert_bit_equal(want, got)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["smallest", "largest"])
@pytest.mark.parametrize("purge_first,mutate", [(True, True), (False, True), (True, False)])
def test_kernel_bit_equal_to_twin_edge_shapes(cuda, shape, purge_first, mutate):
    from avenir_amd.optimize.ga_meeting import ga_meeting_run
    M, Q, dseed, P, m, r, G = _SHAPES[shape]
    if not purge_first and P + r > 64:
        P = 64 - r                                                   # children join the pool: P + r = 64
    _, tb = _instance(M, Q, dseed)
    from avenir_amd.optimize.ga_meeting import ga_meeting_reference
    pop, pc = _start(tb, 3, P, 5, 100)
    want = ga_meeting_reference(tb, pop, pc, G, m, r, purge_first, mutate, 5, 100)
    got = ga_meeting_run(tb, pop, pc, G, m, r, purge_first, mutate, 5, 100, torch.device("cuda"))
    _assert_bit_equal(want, got)


@pytest.mark.gpu
def test_kernel_chunks_equal_one_twin_run(cuda):
    from avenir_amd.optimize.ga_meeting import ga_meeting_reference, ga_meeting_run
    d, tb = _instance(10, 20, 3)
    pop, pc = _start(tb, 7, 30, 9, 40)
    want = ga_meeting_reference(tb, pop, pc, 12, 10, 10, False, True, 9, 40)
    dev = torch.device("cuda")
    a = ga_meeting_run(d, pop, pc, 5, 10, 10, False, True, 9, 40, dev)
    b = ga_meeting_run(d, a[0], a[1], 7, 10, 10, False, True, 9, 40, dev, gen_base=5)
    _assert_bit_equal(want, (b[0], b[1], np.concatenate([a[2], b[2]], 1)))


@pytest.mark.gpu
def test_genetic_algorithm_gpu_equals_cpu(cuda):
    """GeneticAlgorithm takes the kernel on the GPU and the twin on the CPU: same result, migration
    included."""
    from avenir_amd.optimize.search import GeneticAlgorithm
    kw = dict(islands=8, pool=30, mating=10, replacement=10, generations=24, migrate_every=6, purge_first=False,
              use_kernel=True, seed=9)
    rc = GeneticAlgorithm(MeetingScheduleDomain.random_instance(10, 20, seed=3), **kw).run()
    rg = GeneticAlgorithm(MeetingScheduleDomain.random_instance(10, 20, seed=3, device="cuda"), **kw).run()
    assert rg.stats["engine"] == "ga_meeting_kernel" and rc.stats["engine"] == "ga_meeting_twin"
    assert rg.best_cost == rc.best_cost and rg.history == rc.history
    assert torch.equal(rg.best.cpu(), rc.best.cpu())
    assert np.isfinite(rg.best_cost)


@pytest.mark.gpu
def test_default_on_the_gpu_takes_the_kernel(cuda):
    from avenir_amd.optimize.search import GeneticAlgorithm
    d = MeetingScheduleDomain.random_instance(5, 10, seed=2, device="cuda")
    res = GeneticAlgorithm(d, islands=1, pool=16, mating=5, replacement=5, generations=15, seed=2).run()
    assert res.stats["engine"] == "ga_meeting_kernel" and np.isfinite(res.best_cost)
    assert bool(d.valid(res.best.view(1, -1))[0])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["index", "M33", "P_plus_r_65"])
def test_binding_validation(cuda, case):
    """Each violation raises before anything is launched: pop, costs and hist stay as they were."""
    from avenir_amd import _native
    from avenir_amd.optimize.ga_meeting import _device_tables
    _, tb = _instance(10, 20, 3)
    dev = torch.device("cuda")
    P, r, purge = (45, 20, False) if case == "P_plus_r_65" else (30, 10, True)
    pop, pc = _start(tb, 2, P, 1, 0)
    dom = list(_device_tables(tb, dev))
    if case == "index":
        pop = pop.copy()
        pop[1, 3, 4] = tb["cards"][4]                                # an hour index one past its table
    if case == "M33":
        dom[3] = torch.full((33,), 1800, dtype=torch.int32, device=dev)      # dur of 33 meetings
        dom[4] = torch.zeros(33, dtype=torch.int32, device=dev)
        pop = np.zeros((2, P, 99), dtype=np.int16)
    tp, tc = torch.from_numpy(pop).to(dev), torch.from_numpy(pc).to(dev)
    hist = torch.full((2, 3), -1.0, device=dev)
    keep = tp.clone(), tc.clone()
    with pytest.raises((RuntimeError, ValueError)):
        _native.C().ga_meeting(*dom, float("inf"), tp, tc, hist, 3, 10, r, purge, True, 1, 0, 0)
    torch.cuda.synchronize()
    assert torch.equal(tp, keep[0]) and torch.equal(tc, keep[1]) and bool((hist == -1.0).all())
