"""Writes the evolutionary-island fixtures of this folder: assign.npz, meeting.npz and subset.npz.

They record what the host twins of optimize/eo.py (``eo_assign_reference``, ``eo_meeting_reference``, ``eo_subset_reference``)
computed when the island kernels were added; tests/test_eo_golden.py holds every later version of the
twins (on the CPU) and of the kernels (on the GPU) to them.  They are not to be regenerated — code
that disagrees with them has changed.

    python tests/golden/eo_islands/generate.py [assign] [meeting] [subset] [--out DIR]

No fixture depends on a torch or numpy generator's stream: cost tables, conflicts, meeting tables,
priors, labels and every start pool are stored, and the subsets' log-likelihoods are
``float32(-8) * u32_to_unit(Philox(SEED_LL, 0, arange(N F C)).x)``, one fp32 product per entry (the
file keeps their SHA-256).

Layout of a file: ``meta`` is a JSON string {"domains": {name: {scalars, "cases": [parameters]}}};
arrays are keyed ``dom/<domain>/<table>``, ``start/<domain>/<key>/<pop|cost>`` (key = pool size, seed
and island base) and, per case ``i``, ``out/<domain>/<i>/<best|best_cost|stats|pop|cost|born|hist>``: the
outputs of ONE run of ``iters`` iterations.  The same run cut at ``cut`` through the returned state left
the same bits, which the generator asserts; ``stats`` is int64 (inserted, stalls, improved).
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..", "..")))

ISLANDS, ITERS, CUT, SEED_LL = 5, 60, 23, 9
KEYS = ("inserted", "stalls", "improved")
NAMES = ("best", "best_cost", "stats", "pop", "cost", "born", "hist")
# pool, select, w, age_scale, seed, island_base
CASES = [dict(P=5, select=3, w=0.7, age_scale=1.0, seed=5, island_base=0),
         dict(P=5, select=3, w=0.7, age_scale=1.0, seed=5, island_base=100),
         dict(P=10, select=10, w=1.0, age_scale=1.0, seed=6, island_base=0),
         dict(P=10, select=1, w=0.0, age_scale=2.5, seed=7, island_base=0),
         dict(P=2, select=2, w=0.3, age_scale=0.5, seed=8, island_base=3)]


def _save(out, name, meta, arrays):
    path = os.path.join(out, name)
    np.savez_compressed(path, meta=np.array(json.dumps(meta, sort_keys=True)), **arrays)
    print(f"{name}: {os.path.getsize(path)} bytes, {sum(len(d['cases']) for d in meta['domains'].values())} cases")


def _runs(reference, start, arrays, dn):
    """``reference(pop, cost, EoRun, born, best, best_cost)`` over CASES from ``start(P, seed, base)``."""
    from avenir_amd.optimize.eo import EoRun
    for i, c in enumerate(CASES):
        key = f"start/{dn}/{c['P']}-{c['seed']}-{c['island_base']}"
        if key + "/pop" not in arrays:
            arrays[key + "/pop"], arrays[key + "/cost"] = start(c["P"], c["seed"], c["island_base"])
        pop, cost = arrays[key + "/pop"], arrays[key + "/cost"]
        args = (c["select"], c["w"], c["age_scale"], c["seed"])
        one = reference(pop, cost, EoRun(ITERS, *args, 0, c["island_base"]))
        a = reference(pop, cost, EoRun(CUT, *args, 0, c["island_base"]))
        b = reference(a[3], a[4], EoRun(ITERS - CUT, *args, CUT, c["island_base"]), a[5], a[0], a[1])
        two = (b[0], b[1], {k: a[2][k] + b[2][k] for k in KEYS}, b[3], b[4], b[5], np.concatenate([a[6], b[6]], 1))
        for name, x, y in zip(NAMES, one, two):
            if name == "stats":
                assert x == y, (dn, i)
                x = np.array([x[k] for k in KEYS], dtype=np.int64)
            else:
                assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (dn, i, name)
            arrays[f"out/{dn}/{i}/{name}"] = x
        print(dn, i, one[2])


def assign(out):
    from avenir_amd.optimize import AssignmentDomain
    from avenir_amd.optimize.eo import eo_assign_reference
    from avenir_amd.optimize.ga import ga_assign_init
    meta, arrays = {"domains": {}}, {}
    # tests/_eo.py::random_assignment; "crowded" starts with invalid members and stalls often
    for dn, (L, V, seed, density, swap) in {"reference": (24, 10, 0, 0.15, True), "crowded": (6, 4, 1, 0.5, True),
                                            "no-swap": (8, 5, 1, 0.3, False)}.items():
        g = torch.Generator().manual_seed(seed)
        cost = torch.rand((L, V), generator=g) * 100
        conf = torch.rand((L, L), generator=g) < density
        d = AssignmentDomain(cost, conf | conf.T, invalid_cost=1e3, swap_moves=swap)
        arrays[f"dom/{dn}/cost"] = d.cost_table.numpy()
        arrays[f"dom/{dn}/conflict"] = d.conflict.numpy()
        meta["domains"][dn] = {"invalid": 1e3, "swap": swap, "islands": ISLANDS, "iters": ITERS, "cut": CUT,
                               "cases": CASES}
        _runs(lambda *a: eo_assign_reference(d, *a), lambda P, s, b: ga_assign_init(d, ISLANDS, P, s, b), arrays, dn)
    _save(out, "assign.npz", meta, arrays)


_MT_ARRAYS = ("days", "hours", "minutes", "dur", "share", "member", "role_w", "blocked", "ordered", "cards",
              "share_b", "member_b")


def meeting(out):
    from avenir_amd.optimize.domains import MeetingScheduleDomain
    from avenir_amd.optimize.ga_meeting import (eo_meeting_reference, ga_meeting_init, ga_meeting_price,
                                                meeting_tables)
    meta, arrays = {"domains": {}}, {}
    for dn, (M, Q, s) in {"smallest": (1, 3, 0), "reference": (10, 20, 3), "crowded": (32, 40, 0)}.items():
        tb = meeting_tables(MeetingScheduleDomain.random_instance(M, Q, seed=s))
        for k in _MT_ARRAYS:
            arrays[f"dom/{dn}/{k}"] = tb[k]
        meta["domains"][dn] = {"M": tb["M"], "Q": tb["Q"], "L": tb["L"], "invalid": "inf", "islands": ISLANDS,
                               "iters": ITERS, "cut": CUT, "cases": CASES}

        def start(P, seed, base, tb=tb):
            pop = ga_meeting_init(tb, ISLANDS, P, seed, base)
            return pop, ga_meeting_price(tb, pop)

        _runs(lambda *a, tb=tb: eo_meeting_reference(tb, *a), start, arrays, dn)
    _save(out, "meeting.npz", meta, arrays)


def subset_ll(N, F, C):
    from avenir_amd.ops.random import philox4x32, u32_to_unit
    x = philox4x32(SEED_LL, 0, np.arange(N * F * C, dtype=np.uint64))[0]
    return (np.float32(-8.0) * u32_to_unit(x)).astype(np.float32).reshape(N, F, C)


def subset(out):
    from avenir_amd.optimize.domains import FeatureSubsetDomain
    from avenir_amd.optimize.ga_subset import (eo_subset_reference, ga_subset_init, ga_subset_price, pack_masks,
                                               subset_tables)
    meta, arrays = {"domains": {}}, {}
    shapes = {"fixed_size": (517, 12, 3, 5, 5), "short_tile": (300, 32, 16, 1, 32), "reference": (517, 12, 3, 2, 8)}
    for dn, (N, F, C, lo, hi) in shapes.items():                                      # tests/test_eo_subset.py
        LL = subset_ll(N, F, C)
        rng = np.random.default_rng(77 + 100 * F + C)                                 # stored, not replayed
        prior = np.log(rng.dirichlet(np.full(C, 5.0))).astype(np.float32)
        labels = (LL[:, : max(1, F // 3), :].sum(1) + rng.normal(0, 2.0, (N, C))).argmax(1).astype(np.int32)
        labels[0] = C - 1
        arrays[f"dom/{dn}/log_prior"], arrays[f"dom/{dn}/labels"] = prior, labels
        tb = subset_tables(FeatureSubsetDomain(F, loglik=torch.from_numpy(LL), log_prior=torch.from_numpy(prior),
                                               labels=torch.from_numpy(labels), min_size=lo, max_size=hi))
        assert tb is not None and tb["invalid"] == 1.0 and np.array_equal(tb["LL"], LL)
        meta["domains"][dn] = {"N": N, "F": F, "C": C, "min_size": lo, "max_size": hi, "invalid": 1.0,
                               "LL_sha256": hashlib.sha256(LL.tobytes()).hexdigest(), "islands": ISLANDS,
                               "iters": ITERS, "cut": CUT, "cases": CASES}

        def start(P, seed, base, tb=tb):
            pop = ga_subset_init(tb, ISLANDS, P, seed, base)
            return pop, ga_subset_price(tb, pack_masks(pop))

        _runs(lambda *a, tb=tb: eo_subset_reference(tb, *a), start, arrays, dn)
    _save(out, "subset.npz", meta, arrays)


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE
    os.makedirs(out, exist_ok=True)
    which = [a for a in sys.argv[1:] if a in ("assign", "meeting", "subset")] or ["assign", "meeting", "subset"]
    for name in which:
        {"assign": assign, "meeting": meeting, "subset": subset}[name](out)
