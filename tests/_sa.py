"""What the simulated-annealing suites share (test_sa_meeting.py, test_sa_subset.py)."""
import numpy as np


def meeting_start(tb, n, seed, base):
    from avenir_amd.optimize.ga_meeting import ga_meeting_price, sa_meeting_init
    sol = sa_meeting_init(tb, n, seed, base)
    return sol, ga_meeting_price(tb, sol)


def subset_start(tb, n, seed, base):
    from avenir_amd.optimize.ga_subset import ga_subset_price, pack_masks, sa_subset_init
    sol = sa_subset_init(tb, n, seed, base)
    return sol, ga_subset_price(tb, pack_masks(sol))


def state_equal(a, b):
    """(best, best_cost, stats, sol, cost, temperature) bit for bit."""
    for i in (0, 1, 3, 4):
        assert a[i].dtype == b[i].dtype and np.array_equal(a[i], b[i]), i
    assert a[2] == b[2]
    assert np.float32(a[5]).view(np.uint32) == np.float32(b[5]).view(np.uint32)
