"""Feature subsets scored by naive Bayes: the scoring kernel and the island GA as one K22 launch
(csrc/kernels/optim.hip::subset_errors_kernel, ga_subset_kernel) and their numpy twins
(optimize/ga_subset.py).  On the CPU: the scoring twin against an fp64 oracle on exact data,
FeatureSubsetDomain.errors against its GEMM cost, the twin GA's invariants, engine choice in
GeneticAlgorithm.  On the GPU: both kernels bit-equal to the twins, the class equal on both devices."""
import functools

import numpy as np
import pytest
import torch

from avenir_amd.optimize.domains import FeatureSubsetDomain


def _field(F):
    return 0xFFFFFFFF if F == 32 else (1 << F) - 1


@functools.lru_cache(maxsize=None)
def _exact(N, F, C, seed=0, untied=False):
    """LL and priors on the 1/8 grid in [-64, 0]: every sum of up to 33 of them is exact in fp32 in
    any order.  ``untied`` lowers the prior of class c by c / 1024 (still exact: 21 bits), so that no
    two classes of a row can score the same.  The first label is C - 1."""
    rng = np.random.default_rng(1000 * seed + 100 * F + C)
    LL = (rng.integers(0, 513, (N, F, C), dtype=np.int16).astype(np.float32) / np.float32(-8.0))
    prior = (rng.integers(0, 513, C).astype(np.float32) / np.float32(-8.0))
    if untied:
        prior = prior - np.arange(C, dtype=np.float32) / np.float32(1024.0)
    labels = rng.integers(0, C, N)
    labels[0] = C - 1
    return LL, prior, labels


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


def _tables(data, **kw):
    from avenir_amd.optimize.ga_subset import subset_tables
    tb = subset_tables(_domain(data, **kw))
    assert tb is not None
    return tb


def _oracle(data, masks):
    """Independent of the twin: fp64 masked sums, the first maximum over the classes."""
    LL, prior, labels = data
    N, F, C = LL.shape
    out = []
    for mk in masks:
        bits = np.array([(int(mk) >> f) & 1 for f in range(F)], dtype=np.float64)
        s = prior.astype(np.float64)[None, :] + np.einsum("f,nfc->nc", bits, LL.astype(np.float64))
        out.append(int((s.argmax(1) != labels).sum()))
    return np.array(out, dtype=np.int64)


def _masks(F, n, seed):
    """0 (prior only), all ones, bit 31 alone (a stray bit unless F = 32), then random masks."""
    rng = np.random.default_rng(seed)
    rnd = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([np.array([0, 0xFFFFFFFF, 1 << 31], dtype=np.uint32), rnd])


# ------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("N", [1, 257])
@pytest.mark.parametrize("C", [2, 5])
@pytest.mark.parametrize("F", [1, 17, 32])
def test_scoring_twin_matches_fp64_oracle(F, C, N):
    from avenir_amd.optimize.ga_subset import subset_errors, subset_errors_reference
    data = _exact(N, F, C)
    tb = _tables(data)
    masks = _masks(F, 40, seed=F + C)
    got = subset_errors_reference(tb, masks)
    assert got.dtype == np.int64 and got.shape == masks.shape
    assert np.array_equal(got, _oracle(data, masks & np.uint32(_field(F))))
    assert np.array_equal(subset_errors(tb, masks, "cpu"), got)
    if F < 32:
        assert got[2] == got[0]                                       # a bit at or above F is ignored
    assert 0 <= got.min() and got.max() <= N


def test_errors_equal_cost_on_untied_data():
    data = _exact(257, 17, 5, seed=1, untied=True)
    LL, prior, labels = data
    d = _domain(data)
    g = torch.Generator().manual_seed(3)
    sol = torch.randint(0, 2, (64, 17), generator=g)
    sol[0], sol[1] = 0, 1
    # no row has two equal class scores under any of these subsets (fp64, exact on this data)
    s = prior.astype(np.float64)[None, None, :] + np.einsum("pf,nfc->pnc", sol.numpy().astype(np.float64),
                                                            LL.astype(np.float64))
    top = np.sort(s, axis=2)
    assert (top[..., -1] > top[..., -2]).all()
    err = d.errors(sol)
    assert err.dtype == torch.int64 and err.shape == (64,)
    assert torch.equal(err.float() / 257, d.cost(sol))
    assert len(set(err.tolist())) > 8


def _start(tb, I, P, seed, base):
    from avenir_amd.optimize.ga_subset import ga_subset_init, ga_subset_price, pack_masks
    pop = ga_subset_init(tb, I, P, seed, base)
    return pop, ga_subset_price(tb, pack_masks(pop))


def _check_pools(tb, pop, cost):
    """Every member valid and 0 / 1, every stored cost = errors / N priced from scratch."""
    from avenir_amd.optimize.ga_subset import ga_subset_valid, pack_masks, subset_errors_reference
    assert pop.dtype == np.int16 and cost.dtype == np.float32
    assert ((pop == 0) | (pop == 1)).all()
    mk = pack_masks(pop)
    assert ga_subset_valid(tb, mk).all()
    size = pop.sum(-1)
    assert (size >= tb["min_size"]).all() and (size <= tb["max_size"]).all()
    err = subset_errors_reference(tb, mk.reshape(-1)).reshape(mk.shape)
    assert np.array_equal(cost, err.astype(np.float32) / np.float32(tb["N"]))


def test_twin_ga_invariants_chunks_and_global_islands():
    from avenir_amd.optimize.ga_subset import ga_subset_reference
    tb = _tables(_random(257, 17, 5), min_size=2, max_size=9)
    pop, pc = _start(tb, 4, 16, 7, 0)
    _check_pools(tb, pop, pc)
    one = ga_subset_reference(tb, pop, pc, 12, 6, 5, True, True, 7, 0)
    assert one[2].shape == (4, 12) and one[2].dtype == np.float32
    _check_pools(tb, one[0], one[1])
    assert (np.diff(one[2], axis=1) <= 0).all()                       # purge_first, r < P: elitism
    assert (one[2][:, -1] < one[2][:, 0]).any()                       # and the search gets somewhere
    a = ga_subset_reference(tb, pop, pc, 7, 6, 5, True, True, 7, 0)
    _check_pools(tb, a[0], a[1])
    b = ga_subset_reference(tb, a[0], a[1], 5, 6, 5, True, True, 7, 0, gen_base=7)
    assert np.array_equal(one[0], b[0]) and np.array_equal(one[1], b[1])
    assert np.array_equal(one[2], np.concatenate([a[2], b[2]], 1))
    lo = ga_subset_reference(tb, pop[:2], pc[:2], 12, 6, 5, True, True, 7, 0)
    p2, c2 = _start(tb, 2, 16, 7, 2)
    assert np.array_equal(p2, pop[2:]) and np.array_equal(c2, pc[2:])
    hi = ga_subset_reference(tb, p2, c2, 12, 6, 5, True, True, 7, 2)
    for full, x, y in zip(one, lo, hi):
        assert np.array_equal(full, np.concatenate([x, y], 0))
    joined = ga_subset_reference(tb, pop, pc, 6, 6, 5, False, True, 7, 0)   # children join the pool
    _check_pools(tb, joined[0], joined[1])


def test_engine_choice_on_the_cpu():
    from avenir_amd.optimize.search import GeneticAlgorithm
    data = _random(257, 17, 5)
    d = _domain(data, min_size=2, max_size=9)
    kw = dict(islands=2, pool=12, mating=5, replacement=4, generations=6, seed=5)
    twin = GeneticAlgorithm(d, use_kernel=True, **kw).run()
    assert twin.stats.get("engine") == "ga_subset_host"
    assert len(twin.history) == 6
    assert bool(d.valid(twin.best.view(1, -1))[0])
    assert float(d.errors(twin.best.view(1, -1))[0]) / 257 == pytest.approx(float(twin.best_cost), rel=1e-6)
    default = GeneticAlgorithm(d, **kw).run()
    generic = GeneticAlgorithm(d, use_kernel=False, **kw).run()
    assert "engine" not in (default.stats or {}) and "engine" not in (generic.stats or {})
    assert torch.equal(default.best, generic.best) and default.best_cost == generic.best_cost
    assert default.history == generic.history
    # tied groups, a cost callback, a NaN among the log-likelihoods: no subset engine
    LL, prior, labels = data
    grouped = _domain(data, min_size=2, max_size=9, groups=[[0, 1]])
    assert GeneticAlgorithm(grouped, use_kernel=True, **kw)._island_engine() is None
    callback = _domain(data, min_size=2, max_size=9, cost_fn=lambda sol: sol.float().mean(1))
    assert GeneticAlgorithm(callback, use_kernel=True, **kw)._island_engine() is None
    assert "engine" not in (GeneticAlgorithm(callback, use_kernel=True, **kw).run().stats or {})
    bad = LL.copy()
    bad[5, 3, 1] = np.nan
    poisoned = _domain((bad, prior, labels), min_size=2, max_size=9)
    assert GeneticAlgorithm(poisoned, use_kernel=True, **kw)._island_engine() is None
    with pytest.raises(ValueError):
        poisoned.errors(torch.ones((1, 17), dtype=torch.long))


# ------------------------------------------------------------------------------------------- GPU
def _assert_bit_equal(want, got):
    for w, g_ in zip(want, got):
        assert w.dtype == g_.dtype and np.array_equal(w, g_)


def _error_masks(N, F, C, B):
    """B = 1: all ones.  B = 1000: 0, all ones, bit 31, then draws from 997 random masks — from 13
    where one mask costs the twin more than 2^18 adds, so that the twin stays within seconds."""
    if B == 1:
        return np.array([0xFFFFFFFF], dtype=np.uint32)
    pool = _masks(F, 997 if N * F * C <= 1 << 18 else 13, seed=B + F)
    rng = np.random.default_rng(N + C)
    return np.concatenate([pool[:3], pool[rng.integers(0, pool.size, B - 3)]])


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 1000])
@pytest.mark.parametrize("N", [1, 255, 100_003])
@pytest.mark.parametrize("C", [2, 16])
@pytest.mark.parametrize("F", [1, 32])
def test_subset_errors_kernel_equals_twin(cuda, F, C, N, B):
    from avenir_amd.optimize.ga_subset import subset_errors, subset_errors_reference
    data = _exact(N, F, C)
    tb = _tables(data)
    masks = _error_masks(N, F, C, B)
    want = subset_errors_reference(tb, masks)
    got = subset_errors(tb, masks, cuda)
    print(f"F={F} C={C} N={N} B={B}: errors {want.min()}..{want.max()}")
    assert got.dtype == np.int64 and np.array_equal(got, want)
    if N <= 255:
        assert np.array_equal(want, _oracle(data, masks & np.uint32(_field(F))))


@pytest.mark.gpu
def test_subset_errors_kernel_adds_in_feature_order(cuda):
    """Random fp32 values where the order of the adds decides: class 1 holds class 0's values of the
    same row in another feature order, so both scores are the same sum up to rounding."""
    from avenir_amd.optimize.ga_subset import subset_errors, subset_errors_reference
    rng = np.random.default_rng(5)
    N, F = 4099, 32
    base = (-8.0 * rng.random((N, F))).astype(np.float32)
    LL = np.stack([base, base[:, ::-1]], axis=2)                       # [N, F, 2]
    data = (np.ascontiguousarray(LL), np.zeros(2, dtype=np.float32), rng.integers(0, 2, N))
    tb = _tables(data)
    sym = [0xFFFFFFFF, 0x0FFFFFF0, 0x81818181, 0xF00FF00F]              # bit f set iff bit 31 - f is
    masks = np.concatenate([np.array(sym, dtype=np.uint32), _masks(F, 200, seed=9)])
    want = subset_errors_reference(tb, masks)
    # the data discriminates: descending feature order predicts other rows under the symmetric masks
    down = (np.ascontiguousarray(LL[:, ::-1, :]), data[1], data[2])
    rev = [int(f"{m:032b}"[::-1], 2) for m in sym]
    assert np.array_equal(rev, sym)
    assert (subset_errors_reference(_tables(down), np.array(sym, dtype=np.uint32)) != want[:4]).any()
    assert np.array_equal(subset_errors(tb, masks, cuda), want)


_GA = {  # F, C, N, islands, P, m, r, purge_first, mutate, min_size, max_size, G, gen_base
    "F1_N1": (1, 2, 1, 1, 4, 2, 2, True, True, 0, 1, 5, 0),
    "F17_C5_join": (17, 5, 257, 3, 16, 6, 6, False, True, 2, 9, 8, 0),
    "F32_N4099": (32, 2, 4099, 2, 30, 10, 10, True, True, 1, 32, 6, 0),
    "F32_C16_small_tile": (32, 16, 257, 2, 12, 5, 4, True, True, 1, 32, 4, 0),
    "I300": (17, 2, 257, 300, 8, 4, 4, True, True, 2, 9, 4, 0),
    "P64_r32_purge": (17, 5, 257, 2, 64, 20, 32, True, True, 2, 9, 4, 0),
    "P32_r32_join": (17, 5, 257, 2, 32, 32, 32, False, True, 2, 9, 4, 0),
    "m1": (17, 5, 257, 2, 16, 1, 6, True, True, 2, 9, 6, 0),
    "no_mutate": (17, 5, 257, 2, 16, 6, 6, True, False, 2, 9, 6, 0),
    "fixed_size": (17, 5, 257, 2, 16, 6, 6, True, True, 5, 5, 4, 0),
    "gen_base_2p33": (17, 5, 4099, 1, 16, 6, 6, False, True, 2, 9, 5, 1 << 33),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(_GA))
def test_ga_subset_kernel_bit_equal_to_twin(cuda, case):
    from avenir_amd.optimize.ga_subset import ga_subset_reference, ga_subset_run
    F, C, N, I, P, m, r, purge, mutate, lo, hi, G, gen_base = _GA[case]
    data = _random(N, F, C)
    assert (data[2] == C - 1).any()
    tb = _tables(data, min_size=lo, max_size=hi)
    pop, pc = _start(tb, I, P, 5, 100)
    want = ga_subset_reference(tb, pop, pc, G, m, r, purge, mutate, 5, 100, gen_base)
    if case == "fixed_size":       # a flip of a child of size 5 leaves the range: retries run out, it costs 1.0
        assert (want[1] == 1.0).any() and np.array_equal(want[1] == 1.0, want[0].sum(-1) != 5)
    elif case != "F1_N1":
        assert not np.array_equal(want[0], pop)
    got = ga_subset_run(tb, pop, pc, G, m, r, purge, mutate, 5, 100, cuda, gen_base=gen_base)
    _assert_bit_equal(want, got)


@pytest.mark.gpu
def test_ga_subset_kernel_chunks_equal_one_twin_run(cuda):
    from avenir_amd.optimize.ga_subset import ga_subset_reference, ga_subset_run
    tb = _tables(_random(257, 17, 5), min_size=2, max_size=9)
    pop, pc = _start(tb, 4, 16, 7, 0)
    want = ga_subset_reference(tb, pop, pc, 12, 6, 5, True, True, 7, 0)
    a = ga_subset_run(tb, pop, pc, 7, 6, 5, True, True, 7, 0, cuda)
    b = ga_subset_run(tb, a[0], a[1], 5, 6, 5, True, True, 7, 0, cuda, gen_base=7)
    _assert_bit_equal(want, (b[0], b[1], np.concatenate([a[2], b[2]], 1)))
    lo = ga_subset_run(tb, pop[:2], pc[:2], 12, 6, 5, True, True, 7, 0, cuda)
    hi = ga_subset_run(tb, pop[2:], pc[2:], 12, 6, 5, True, True, 7, 2, cuda)
    _assert_bit_equal(want, [np.concatenate([x, y], 0) for x, y in zip(lo, hi)])


@pytest.mark.gpu
def test_genetic_algorithm_on_churn_gpu_equals_cpu(cuda, tmp_path):
    from avenir_amd.data import synth
    from avenir_amd.data.table import load_csv
    from avenir_amd.models.bayes import NaiveBayes
    from avenir_amd.optimize.search import GeneticAlgorithm
    from avenir_amd.utils.schema import FeatureSchema
    p = tmp_path / "churn.csv"
    synth.write_churn(p, 4000, seed=2)
    t = load_csv(p, FeatureSchema.from_json(synth.CHURN_SCHEMA), device=cuda)
    nb = NaiveBayes().fit(t)
    d = FeatureSubsetDomain.from_naive_bayes(nb, t, t.labels[: t.n], min_size=1)
    assert d.device.type == "cuda" and d.loglik.shape[0] == 4000
    kw = dict(islands=2, pool=16, mating=6, replacement=6, generations=20)
    rg = GeneticAlgorithm(d, **kw).run()
    assert rg.stats["engine"] == "ga_subset_kernel"
    assert bool(d.valid(rg.best.view(1, -1))[0])
    all_on = torch.ones((1, d.F), dtype=torch.long, device=cuda)
    assert rg.best_cost <= float(d.cost(all_on))
    assert float(d.errors(rg.best.view(1, -1))[0]) / 4000 == pytest.approx(rg.best_cost, rel=1e-6)
    dc = FeatureSubsetDomain(d.F, min_size=1, loglik=d.loglik.cpu(), log_prior=d.log_prior.cpu(), labels=d.labels.cpu())
    rc = GeneticAlgorithm(dc, use_kernel=True, **kw).run()
    assert rc.stats["engine"] == "ga_subset_host"
    assert rg.best_cost == rc.best_cost and rg.history == rc.history
    assert torch.equal(rg.best.cpu(), rc.best) and torch.equal(rg.costs.cpu(), rc.costs)
