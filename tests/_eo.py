"""What the evolutionary-island suites share (test_eo_islands.py, test_eo_meeting.py, test_eo_golden.py)."""
import numpy as np
import torch

from avenir_amd.optimize import AssignmentDomain
from avenir_amd.optimize.eo import EoRun

NAMES = ("best", "best_cost", "stats", "pop", "cost", "born", "hist")
COUNTERS = ("inserted", "stalls", "improved")


def random_assignment(L=24, V=10, seed=0, density=0.15):
    """The ``_random_assignment`` of test_optimize.py."""
    g = torch.Generator().manual_seed(seed)
    cost = torch.rand((L, V), generator=g) * 100
    conf = torch.rand((L, L), generator=g) < density
    conf = conf | conf.T
    return AssignmentDomain(cost, conf, invalid_cost=1e3)


def assign_start(d, n, P, seed, base=0):
    from avenir_amd.optimize.ga import ga_assign_init
    return ga_assign_init(d, n, P, seed, base)


def meeting_start(tb, n, P, seed, base=0):
    from avenir_amd.optimize.ga_meeting import ga_meeting_init, ga_meeting_price
    pop = ga_meeting_init(tb, n, P, seed, base)
    return pop, ga_meeting_price(tb, pop)


def assert_same(a, b):
    """(best, best_cost, stats, pop, cost, born, hist) bit for bit, dtypes included."""
    for name, x, y in zip(NAMES, a, b):
        if name == "stats":
            assert x == y, (x, y)
            continue
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, (name, x.shape, y.shape, x.dtype, y.dtype)
        if x.dtype.kind == "f":
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), name
        else:
            assert np.array_equal(x, y), name


def segments(advance, pop, cost, run: EoRun, step: int, check=None):
    """``advance(pop, cost, EoRun, born=, best=, best_cost=)`` over ``run`` cut every ``step`` iterations
    through the returned state -> the outputs of one run; ``check(before, after)`` sees every segment."""
    state = {}
    stats = dict.fromkeys(COUNTERS, 0)
    hists = []
    out = None
    for b in range(run.it_begin, run.it_begin + run.iters, step):
        n = min(step, run.it_begin + run.iters - b)
        before = (pop, cost, state.get("born"))
        out = advance(pop, cost, EoRun(n, run.select, run.w, run.age_scale, run.seed, b, run.island_base), **state)
        best, bc, st, pop, cost, born, h = out
        if check is not None:
            check(before, out)
        state = {"born": born, "best": best, "best_cost": bc}
        hists.append(np.asarray(h))
        for k in stats:
            stats[k] += st[k]
    return out[0], out[1], stats, out[3], out[4], out[5], np.concatenate(hists, 1)


def check_invariants(price, P, before, after):
    """After a segment: every member's cost is the domain price of the member, stamps are distinct,
    exactly one slot changed per inserted iteration (by the stamps), ``hist`` never rises and ends at
    ``best_cost``, which is the price of ``best``."""
    best, bc, st, pop, cost, born, hist = (x if isinstance(x, dict) else np.asarray(x) for x in after)
    assert np.array_equal(price(pop.astype(np.int64)).view(np.uint32), cost.view(np.uint32))
    assert all(np.unique(row).size == P for row in born)
    b0 = np.broadcast_to(np.arange(P, dtype=np.int32), born.shape) if before[2] is None else np.asarray(before[2])
    changed = born != b0
    assert int(changed.sum()) <= st["inserted"]              # a slot replaced twice shows once
    if hist.shape[1] == 1:                                    # one iteration: one slot per inserting island
        assert int(changed.sum()) == st["inserted"] and (changed.sum(1) <= 1).all()
    assert np.array_equal(pop[~changed], np.asarray(before[0])[~changed])
    assert np.array_equal(cost[~changed], np.asarray(before[1])[~changed])
    if hist.shape[1]:
        assert (hist[:, 1:] <= hist[:, :-1]).all()                # costs may be inf: no differences
        assert np.array_equal(hist[:, -1].view(np.uint32), bc.view(np.uint32))
    assert np.array_equal(price(best.astype(np.int64)).view(np.uint32), bc.view(np.uint32))
