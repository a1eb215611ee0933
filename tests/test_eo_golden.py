"""The frozen evolutionary-island fixtures of tests/golden/eo_islands (written by its generate.py): the host
twins of optimize/eo.py replay them on the CPU, ``eo_assign_kernel``, ``eo_meeting_kernel`` and ``eo_subset_kernel``
on the GPU, as one run and as two segments, bit for bit in every output."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from avenir_amd.optimize.eo import EoRun

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eo_islands")
_KEYS = ("inserted", "stalls", "improved")
_NAMES = ("best", "best_cost", "stats", "pop", "cost", "born", "hist")


@functools.lru_cache(maxsize=None)
def _load(name):
    with np.load(os.path.join(_DIR, name + ".npz"), allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    return json.loads(str(arrays.pop("meta"))), arrays


def _cases(name):
    return [(dn, i) for dn, d in sorted(_load(name)[0]["domains"].items()) for i in range(len(d["cases"]))]


def _dom(arrays, dn):
    pre = f"dom/{dn}/"
    return {k[len(pre):]: v for k, v in arrays.items() if k.startswith(pre)}


def _assert_frozen(name, dn, i, advance):
    """``advance(pop, cost, EoRun, born, best, best_cost)`` as one run and as two segments against case i."""
    meta, arrays = _load(name)
    s = meta["domains"][dn]
    c = s["cases"][i]
    key = f"start/{dn}/{c['P']}-{c['seed']}-{c['island_base']}"
    pop, cost = arrays[key + "/pop"], arrays[key + "/cost"]
    args = (c["select"], c["w"], c["age_scale"], c["seed"])
    one = advance(pop, cost, EoRun(s["iters"], *args, 0, c["island_base"]), None, None, None)
    a = advance(pop, cost, EoRun(s["cut"], *args, 0, c["island_base"]), None, None, None)
    b = advance(a[3], a[4], EoRun(s["iters"] - s["cut"], *args, s["cut"], c["island_base"]), a[5], a[0], a[1])
    two = (b[0], b[1], {k: a[2][k] + b[2][k] for k in _KEYS}, b[3], b[4], b[5], np.concatenate([a[6], b[6]], 1))
    for got in (one, two):
        for n, x in zip(_NAMES, got):
            want = arrays[f"out/{dn}/{i}/{n}"]
            if n == "stats":
                assert [x[k] for k in _KEYS] == want.tolist()
            else:
                assert x.dtype == want.dtype and x.shape == want.shape, n
                assert np.array_equal(x.view(np.uint8), want.view(np.uint8)), n


def _assign_domain(dn):
    import torch
    from avenir_amd.optimize import AssignmentDomain
    meta, arrays = _load("assign")
    s = meta["domains"][dn]
    return AssignmentDomain(torch.from_numpy(arrays[f"dom/{dn}/cost"]), torch.from_numpy(arrays[f"dom/{dn}/conflict"]),
                            invalid_cost=s["invalid"], swap_moves=s["swap"])


def _meeting_tables(dn):
    meta, arrays = _load("meeting")
    s = meta["domains"][dn]
    return dict(_dom(arrays, dn), M=s["M"], Q=s["Q"], L=s["L"], invalid=float(s["invalid"]))


@functools.lru_cache(maxsize=None)
def _subset_tables(dn):
    from avenir_amd.ops.random import philox4x32, u32_to_unit
    meta, arrays = _load("subset")
    s = meta["domains"][dn]
    x = philox4x32(9, 0, np.arange(s["N"] * s["F"] * s["C"], dtype=np.uint64))[0]
    LL = (np.float32(-8.0) * u32_to_unit(x)).astype(np.float32).reshape(s["N"], s["F"], s["C"])
    assert hashlib.sha256(LL.tobytes()).hexdigest() == s["LL_sha256"]
    return dict(_dom(arrays, dn), LL=LL, **{k: s[k] for k in ("N", "F", "C", "min_size", "max_size", "invalid")})


@pytest.mark.parametrize("dn,i", _cases("assign"))
def test_assign_twin_equals_frozen(dn, i):
    from avenir_amd.optimize.eo import eo_assign_reference
    d = _assign_domain(dn)
    _assert_frozen("assign", dn, i, lambda *a: eo_assign_reference(d, *a))


@pytest.mark.parametrize("dn,i", _cases("meeting"))
def test_meeting_twin_equals_frozen(dn, i):
    from avenir_amd.optimize.ga_meeting import eo_meeting_reference
    tb = _meeting_tables(dn)
    _assert_frozen("meeting", dn, i, lambda *a: eo_meeting_reference(tb, *a))


@pytest.mark.parametrize("dn,i", _cases("subset"))
def test_subset_twin_equals_frozen(dn, i):
    from avenir_amd.optimize.ga_subset import eo_subset_advance
    tb = _subset_tables(dn)
    _assert_frozen("subset", dn, i, lambda pop, cost, run, *st: eo_subset_advance(tb, pop, cost, run, "cpu", *st))


def test_the_frozen_cases_take_every_branch():
    for name in ("assign", "meeting", "subset"):
        meta, arrays = _load(name)
        tot = np.zeros(3, dtype=np.int64)
        for dn, i in _cases(name):
            tot += arrays[f"out/{dn}/{i}/stats"]
        assert (tot > 0).all(), (name, tot)
        assert os.path.getsize(os.path.join(_DIR, name + ".npz")) < 100 * 1024


@pytest.mark.gpu
@pytest.mark.parametrize("dn,i", _cases("assign"))
def test_assign_kernel_equals_frozen(cuda, dn, i):
    from avenir_amd.optimize.eo import eo_assign_advance
    d = _assign_domain(dn).to(cuda)
    _assert_frozen("assign", dn, i, lambda pop, cost, run, *st: eo_assign_advance(d, pop, cost, run, cuda, *st))


@pytest.mark.gpu
@pytest.mark.parametrize("dn,i", _cases("meeting"))
def test_meeting_kernel_equals_frozen(cuda, dn, i):
    from avenir_amd.optimize.ga_meeting import eo_meeting_advance
    tb = _meeting_tables(dn)
    _assert_frozen("meeting", dn, i, lambda pop, cost, run, *st: eo_meeting_advance(tb, pop, cost, run, cuda, *st))


@pytest.mark.gpu
@pytest.mark.parametrize("dn,i", _cases("subset"))
def test_subset_kernel_equals_frozen(cuda, dn, i):
    from avenir_amd.optimize.ga_subset import eo_subset_advance
    tb = _subset_tables(dn)
    _assert_frozen("subset", dn, i, lambda pop, cost, run, *st: eo_subset_advance(tb, pop, cost, run, cuda, *st))
