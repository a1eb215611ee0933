"""Writes the island-GA fixtures of this folder: assign.npz, meeting.npz, subset.npz.

Run ONCE at commit 962ddc9 ("Island GA kernel for feature subsets with naive-Bayes scoring"), before
the three host twins (optimize/ga.py, ga_meeting.py, ga_subset.py) were rebuilt on one shared frame:
the files record what the twins computed then, and tests/test_ga_golden.py holds every later
version to it.  They are not to be regenerated — a twin that disagrees with them has changed.

    python tests/golden/ga_islands/generate.py

Every array that does not come from Philox (cost tables, conflicts, the meeting tables, LL, priors,
labels) is stored, so no fixture depends on a torch or numpy generator's stream.  Layout of a file:
``meta`` is a JSON string {"domains": {name: scalars}, "cases": {name: parameters}, "init": {...}};
arrays are keyed ``dom/<domain>/<field>``, ``start/<start>/<pop0|pc0>`` (the initial pools and costs;
cases that begin alike name the same start), ``case/<case>/<pop|pc|hist>`` and ``init/pop``.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..", "..")))

I = 3            # islands of every case
SEED, BASE = 5, 100


def _save(name, meta, arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, meta=np.array(json.dumps(meta, sort_keys=True)), **arrays)
    print(f"{name}: {os.path.getsize(path)} bytes, {len(meta['cases'])} cases")


def _case(arrays, name, start, pop0, pc0, out):
    for k, v in (("pop0", pop0), ("pc0", pc0)):
        key = f"start/{start}/{k}"
        assert key not in arrays or np.array_equal(arrays[key], v)
        arrays[key] = v
    for k, v in zip(("pop", "pc", "hist"), out):
        arrays[f"case/{name}/{k}"] = v


def assign():
    from avenir_amd.optimize.domain import AssignmentDomain
    from avenir_amd.optimize.ga import ga_assign_reference, ga_init_population, ga_price

    def domain(L, V, seed=3):                      # the domain of tests/test_ga_kernel.py
        g = torch.Generator().manual_seed(seed)
        cost = torch.rand((L, V), generator=g) * 100
        conf = torch.rand((L, L), generator=g) < 0.1
        d = AssignmentDomain(cost, conf | conf.T, invalid_cost=150.0)
        return d.cost_table.numpy().astype(np.float32), d.conflict.numpy()

    meta = {"domains": {}, "cases": {}, "init": {}}
    arrays = {}
    for dn, (L, V) in {"L24_V9": (24, 9), "L1_V2": (1, 2)}.items():
        cost, conf = domain(L, V)
        arrays[f"dom/{dn}/cost"], arrays[f"dom/{dn}/conflict"] = cost, conf
        meta["domains"][dn] = {"invalid": 150.0}
    # name: domain, P, m, r, purge_first, mutate, swap, conflict?, G, gen_base
    cases = {
        "purge_mutate": ("L24_V9", 20, 8, 6, True, True, True, True, 8, 0),
        "join_mutate": ("L24_V9", 20, 8, 6, False, True, True, True, 8, 0),
        "purge_no_mutate": ("L24_V9", 20, 8, 6, True, False, True, True, 8, 0),
        "no_swap": ("L24_V9", 20, 8, 6, True, True, False, True, 8, 0),
        "no_conflict": ("L24_V9", 20, 8, 6, True, True, True, False, 8, 0),
        "L1_V2": ("L1_V2", 6, 3, 2, True, True, True, True, 6, 0),
        "P2": ("L24_V9", 2, 1, 1, True, True, True, True, 8, 0),
        "P64_r32_purge": ("L24_V9", 64, 20, 32, True, True, True, True, 4, 0),
        "P40_r24_join": ("L24_V9", 40, 12, 24, False, True, True, True, 4, 0),
        "gen_base_5": ("L24_V9", 20, 8, 6, True, True, True, True, 6, 5),
        "gen_base_2p33": ("L24_V9", 20, 8, 6, False, True, True, True, 6, 1 << 33),
    }
    for name, (dn, P, m, r, purge, mutate, swap, use_conf, G, gen_base) in cases.items():
        cost = arrays[f"dom/{dn}/cost"]
        conf = arrays[f"dom/{dn}/conflict"] if use_conf else None
        L, V = cost.shape
        pop0 = ga_init_population(I, P, L, V, SEED, BASE, conf)
        pc0 = ga_price(cost, conf, 150.0, pop0.astype(np.int64))
        out = ga_assign_reference(cost, conf, 150.0, pop0, pc0, G, m, r, purge, mutate, SEED, BASE, gen_base, swap)
        start = f"{dn}_P{P}" + ("" if use_conf else "_free")
        _case(arrays, name, start, pop0, pc0, out)
        meta["cases"][name] = dict(domain=dn, start=start, P=P, m=m, r=r, purge_first=purge, mutate=mutate, swap=swap,
                                   conflict=use_conf, G=G, gen_base=gen_base, seed=SEED, island_base=BASE)
    meta["init"] = dict(domain="L24_V9", islands=4, P=7, seed=11, island_base=3)
    arrays["init/pop"] = ga_init_population(4, 7, 24, 9, 11, 3, arrays["dom/L24_V9/conflict"])
    _save("assign.npz", meta, arrays)


_MT_ARRAYS = ("days", "hours", "minutes", "dur", "share", "member", "role_w", "blocked", "ordered", "cards",
              "share_b", "member_b")


def meeting():
    from avenir_amd.optimize.domains import MeetingScheduleDomain
    from avenir_amd.optimize.ga_meeting import (ga_meeting_init, ga_meeting_price, ga_meeting_reference,
                                                meeting_tables)
    meta = {"domains": {}, "cases": {}, "init": {}}
    arrays = {}
    tabs = {}

    def add(dn, d):
        tb = meeting_tables(d)
        assert tb is not None
        tabs[dn] = tb
        for k in _MT_ARRAYS:
            arrays[f"dom/{dn}/{k}"] = tb[k]
        meta["domains"][dn] = {"M": tb["M"], "Q": tb["Q"], "L": tb["L"], "invalid": "inf"}

    # the shapes of tests/test_ga_meeting.py: M, Q, domain seed
    for dn, (M, Q, s) in {"smallest": (1, 3, 0), "reference": (10, 20, 3), "largest": (32, 64, 2)}.items():
        add(dn, MeetingScheduleDomain.random_instance(M, Q, seed=s))
    src = MeetingScheduleDomain.random_instance(5, 10, seed=0)
    parts = [src.member[:, i].nonzero().view(-1).tolist() for i in range(5)]
    add("one_minute", MeetingScheduleDomain(parts, (src.dur / 60).tolist(), 10, src.ordered, src.blocked,
                                            src.role_w.tolist(), minutes=(0,)))
    assert tabs["one_minute"]["cards"][2] == 1
    # domain: P, m, r, G (the test's shapes at <= 8 generations)
    shapes = {"smallest": (2, 1, 1, 5), "reference": (30, 10, 10, 8), "largest": (64, 20, 32, 4)}
    cases = {}
    for dn, (P, m, r, G) in shapes.items():
        cases[f"{dn}_purge"] = (dn, P, m, r, True, G)
        cases[f"{dn}_join"] = (dn, min(P, 64 - r), m, r, False, G)     # children join the pool: P + r <= 64
    cases["one_minute"] = ("one_minute", 12, 6, 4, False, 6)
    for name, (dn, P, m, r, purge, G) in cases.items():
        tb = tabs[dn]
        pop0 = ga_meeting_init(tb, I, P, SEED, BASE)
        pc0 = ga_meeting_price(tb, pop0)
        out = ga_meeting_reference(tb, pop0, pc0, G, m, r, purge, True, SEED, BASE)
        _case(arrays, name, f"{dn}_P{P}", pop0, pc0, out)
        meta["cases"][name] = dict(domain=dn, start=f"{dn}_P{P}", P=P, m=m, r=r, purge_first=purge, mutate=True, G=G, gen_base=0,
                                   seed=SEED, island_base=BASE)
    meta["init"] = dict(domain="reference", islands=4, P=7, seed=11, island_base=3)
    arrays["init/pop"] = ga_meeting_init(tabs["reference"], 4, 7, 11, 3)
    _save("meeting.npz", meta, arrays)


def subset():
    from avenir_amd.optimize.domains import FeatureSubsetDomain
    from avenir_amd.optimize.ga_subset import (ga_subset_init, ga_subset_price, ga_subset_reference, pack_masks,
                                               subset_tables)
    meta = {"domains": {}, "cases": {}, "init": {}}
    arrays = {}

    def data(N, F, C):                            # as tests/test_ga_subset.py::_random
        rng = np.random.default_rng(77 + 100 * F + C)
        LL = (-8.0 * rng.random((N, F, C))).astype(np.float32)
        prior = np.log(rng.dirichlet(np.full(C, 5.0))).astype(np.float32)
        labels = (LL[:, : max(1, F // 3), :].sum(1) + rng.normal(0, 2.0, (N, C))).argmax(1)
        labels[0] = C - 1
        return LL, prior, labels

    for dn, (N, F, C) in {"F1_N1": (1, 1, 2), "F9": (33, 9, 3), "F32": (17, 32, 2)}.items():
        LL, prior, labels = data(N, F, C)
        arrays[f"dom/{dn}/LL"], arrays[f"dom/{dn}/log_prior"] = LL, prior
        arrays[f"dom/{dn}/labels"] = labels.astype(np.int32)
        meta["domains"][dn] = {"N": N, "F": F, "C": C, "invalid": 1.0}
    # name: domain, P, m, r, purge_first, mutate, min_size, max_size, G, gen_base
    cases = {
        "F1_N1": ("F1_N1", 4, 2, 2, True, True, 0, 1, 5, 0),
        "F32": ("F32", 30, 10, 10, True, True, 1, 32, 6, 0),
        "fixed_size": ("F9", 16, 6, 6, True, True, 4, 4, 4, 0),
        "join": ("F9", 16, 6, 6, False, True, 2, 6, 8, 0),
        "gen_base_2p33": ("F9", 16, 6, 6, False, True, 2, 6, 5, 1 << 33),
    }
    for name, (dn, P, m, r, purge, mutate, lo, hi, G, gen_base) in cases.items():
        LL, prior, labels = (arrays[f"dom/{dn}/{k}"] for k in ("LL", "log_prior", "labels"))
        tb = subset_tables(FeatureSubsetDomain(LL.shape[1], loglik=torch.from_numpy(LL),
                                               log_prior=torch.from_numpy(prior), labels=torch.from_numpy(labels),
                                               min_size=lo, max_size=hi))
        assert tb is not None and tb["invalid"] == 1.0
        pop0 = ga_subset_init(tb, I, P, SEED, BASE)
        pc0 = ga_subset_price(tb, pack_masks(pop0))
        out = ga_subset_reference(tb, pop0, pc0, G, m, r, purge, mutate, SEED, BASE, gen_base)
        start = f"{dn}_P{P}_{lo}_{hi}"
        _case(arrays, name, start, pop0, pc0, out)
        meta["cases"][name] = dict(domain=dn, start=start, P=P, m=m, r=r, purge_first=purge, mutate=mutate, min_size=lo,
                                   max_size=hi, G=G, gen_base=gen_base, seed=SEED, island_base=BASE)
        if name == "join":
            meta["init"] = dict(case="join", islands=4, P=7, seed=11, island_base=3)
            arrays["init/pop"] = ga_subset_init(tb, 4, 7, 11, 3)
    _save("subset.npz", meta, arrays)


if __name__ == "__main__":
    assign()
    meeting()
    subset()
