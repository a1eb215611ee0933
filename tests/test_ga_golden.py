"""The three island-GA host twins against outputs frozen before they shared one frame
(tests/golden/ga_islands/*.npz, written by generate.py there at the commit its docstring names).
The kernels are tested against the twins, so this is what keeps twin and kernel from drifting
together: every stored case replays bit for bit, dtypes included."""
import functools
import json
import os

import numpy as np
import pytest

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ga_islands")


@functools.lru_cache(maxsize=None)
def _load(name):
    with np.load(os.path.join(_DIR, name + ".npz"), allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    return json.loads(str(arrays.pop("meta"))), arrays


def _cases(name):
    return sorted(_load(name)[0]["cases"])


def _dom(arrays, dn):
    pre = f"dom/{dn}/"
    return {k[len(pre):]: v for k, v in arrays.items() if k.startswith(pre)}


def _start(arrays, c):
    return arrays[f"start/{c['start']}/pop0"], arrays[f"start/{c['start']}/pc0"]


def _assert_case(arrays, case, got):
    for k, g in zip(("pop", "pc", "hist"), got):
        want = arrays[f"case/{case}/{k}"]
        assert g.dtype == want.dtype and g.shape == want.shape and np.array_equal(g, want), k
    assert got[0].dtype == np.int16 and got[1].dtype == np.float32 and got[2].dtype == np.float32


def _meeting_tables(meta, arrays, dn):
    tb = _dom(arrays, dn)
    s = meta["domains"][dn]
    tb.update(M=s["M"], Q=s["Q"], L=s["L"], invalid=float(s["invalid"]))
    return tb


def _subset_tables(meta, arrays, dn, lo, hi):
    tb = _dom(arrays, dn)
    s = meta["domains"][dn]
    tb.update(N=s["N"], F=s["F"], C=s["C"], min_size=lo, max_size=hi, invalid=float(s["invalid"]))
    return tb


@pytest.mark.parametrize("case", _cases("assign"))
def test_assign_twin_equals_frozen(case):
    from avenir_amd.optimize.ga import ga_assign_reference, ga_init_population, ga_price
    meta, arrays = _load("assign")
    c = meta["cases"][case]
    dom = _dom(arrays, c["domain"])
    cost, conf = dom["cost"], dom["conflict"] if c["conflict"] else None
    pop0, pc0 = _start(arrays, c)
    init = ga_init_population(pop0.shape[0], c["P"], cost.shape[0], cost.shape[1], c["seed"], c["island_base"], conf)
    assert init.dtype == pop0.dtype and np.array_equal(init, pop0)
    price = ga_price(cost, conf, 150.0, pop0.astype(np.int64))
    assert price.dtype == pc0.dtype and np.array_equal(price, pc0)
    got = ga_assign_reference(cost, conf, 150.0, pop0, pc0, c["G"], c["m"], c["r"], c["purge_first"], c["mutate"],
                              c["seed"], c["island_base"], c["gen_base"], c["swap"])
    _assert_case(arrays, case, got)


@pytest.mark.parametrize("case", _cases("meeting"))
def test_meeting_twin_equals_frozen(case):
    from avenir_amd.optimize.ga_meeting import ga_meeting_init, ga_meeting_price, ga_meeting_reference
    meta, arrays = _load("meeting")
    c = meta["cases"][case]
    tb = _meeting_tables(meta, arrays, c["domain"])
    pop0, pc0 = _start(arrays, c)
    init = ga_meeting_init(tb, pop0.shape[0], c["P"], c["seed"], c["island_base"])
    assert init.dtype == pop0.dtype and np.array_equal(init, pop0)
    price = ga_meeting_price(tb, pop0)
    assert price.dtype == pc0.dtype and np.array_equal(price, pc0)
    got = ga_meeting_reference(tb, pop0, pc0, c["G"], c["m"], c["r"], c["purge_first"], c["mutate"], c["seed"],
                               c["island_base"], c["gen_base"])
    _assert_case(arrays, case, got)


@pytest.mark.parametrize("case", _cases("subset"))
def test_subset_twin_equals_frozen(case):
    from avenir_amd.optimize.ga_subset import ga_subset_init, ga_subset_price, ga_subset_reference, pack_masks
    meta, arrays = _load("subset")
    c = meta["cases"][case]
    tb = _subset_tables(meta, arrays, c["domain"], c["min_size"], c["max_size"])
    pop0, pc0 = _start(arrays, c)
    init = ga_subset_init(tb, pop0.shape[0], c["P"], c["seed"], c["island_base"])
    assert init.dtype == pop0.dtype and np.array_equal(init, pop0)
    price = ga_subset_price(tb, pack_masks(pop0))
    assert price.dtype == pc0.dtype and np.array_equal(price, pc0)
    got = ga_subset_reference(tb, pop0, pc0, c["G"], c["m"], c["r"], c["purge_first"], c["mutate"], c["seed"],
                              c["island_base"], c["gen_base"])
    _assert_case(arrays, case, got)


def test_initial_pools_equal_frozen():
    from avenir_amd.optimize.ga import ga_init_population
    from avenir_amd.optimize.ga_meeting import ga_meeting_init
    from avenir_amd.optimize.ga_subset import ga_subset_init
    meta, arrays = _load("assign")
    i, dom = meta["init"], _dom(arrays, meta["init"]["domain"])
    got = ga_init_population(i["islands"], i["P"], *dom["cost"].shape, i["seed"], i["island_base"], dom["conflict"])
    assert got.dtype == np.int16 and np.array_equal(got, arrays["init/pop"])
    meta, arrays = _load("meeting")
    i = meta["init"]
    got = ga_meeting_init(_meeting_tables(meta, arrays, i["domain"]), i["islands"], i["P"], i["seed"], i["island_base"])
    assert got.dtype == np.int16 and np.array_equal(got, arrays["init/pop"])
    meta, arrays = _load("subset")
    i = meta["init"]
    c = meta["cases"][i["case"]]
    tb = _subset_tables(meta, arrays, c["domain"], c["min_size"], c["max_size"])
    got = ga_subset_init(tb, i["islands"], i["P"], i["seed"], i["island_base"])
    assert got.dtype == np.int16 and np.array_equal(got, arrays["init/pop"])
