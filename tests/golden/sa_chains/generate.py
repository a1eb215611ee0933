"""Writes the simulated-annealing fixtures of this folder: meeting.npz, subset.npz, assign.npz and,
with ``--gpu`` on an MI355X, assign_gpu.npz.

Run ONCE at commit f4eadc2 ("One-launch SA kernels for meeting-schedule and feature-subset domains"),
before the assignment path's launcher, binding and engine joined the frame of the other two: the files
record what the twins and the assignment kernel computed then, and tests/test_sa_golden.py holds
every later version to it.  They are not to be regenerated — code that disagrees with them has changed.

    python tests/golden/sa_chains/generate.py [--gpu] [--out DIR]

No fixture depends on a torch or numpy generator's stream: cost tables, conflicts, meeting tables,
priors, labels and every start are stored, and the subsets' log-likelihoods are
``float32(-8) * u32_to_unit(Philox(SEED_LL, 0, arange(N F C)).x)``, one fp32 product per entry (the
file keeps their SHA-256).

Layout of a file: ``meta`` is a JSON string {"dtypes": [...], "domains": {name: {scalars, "cases":
[parameters]}}}; arrays are keyed ``dom/<domain>/<table>``, ``start/<domain>/<key>/<sol|cost>`` and,
stacked over the domain's cases in the order of ``cases``, ``out/<domain>/<sols|costs|scal>``:

* meeting, subset, assign — ``sols`` [case, 2, 2, P, L] (one run | two segments; best, sol), ``costs``
  [case, 2, 2, P] (best_cost, cost) and ``scal`` int64 [case, 2, 4] (better, worse_accepted, rejected —
  summed over the segments — and the bits of the temperature).  The second segment starts at move
  ``cut``.  ``dtypes`` are those of (best, best_cost, sol, cost, temperature) as returned.
* assign_gpu — ``sols`` [case, 2, 65, L] (best and sol MINUS the start, which 100 moves leave mostly
  zero; rows past the case's chains are zero) and ``costs`` [case, 2, 65] after ``moves`` moves: one
  launch and two launches (cut at ``cut``) left the same bits, which the generator asserts; ``scal``
  [case, 3, 4] is stats[0..3] of the one launch and of each of the two.

``sa_assign_reference`` prices a worse move with float32 ``np.exp``, whose last bit may differ between
CPUs' SIMD paths.  Each assign case is therefore run three times — as is, with ``np.exp`` moved one
ulp up and one ulp down — and kept only when all three outputs are identical; otherwise the next seed
is tried.  Every case below passed with its first seed (1 seed tried per case), which the generator
asserts, so the stored seeds are the ones named here.
"""
import hashlib
import itertools
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..", "..")))

SEED, BASE, OFFSET, SEED_LL = 5, 100, 17, 9
P, MOVES, CUT, INTERVAL = 5, 40, 17, 3            # the host twins' chains, moves and second segment
KEYS = ("better", "worse_accepted", "rejected")


def _bits(temp) -> int:
    return int(np.float32(temp).view(np.uint32))


def _save(out, name, meta, arrays):
    path = os.path.join(out, name)
    np.savez_compressed(path, meta=np.array(json.dumps(meta, sort_keys=True)), **arrays)
    print(f"{name}: {os.path.getsize(path)} bytes, {sum(len(d['cases']) for d in meta['domains'].values())} cases")


def _segments(run, sol, cost, moves, cut):
    """``run(sol, cost, iters, it_begin, temp_start, best, best_cost)`` as one call and as two."""
    one = run(sol, cost, moves, 0, None, None, None)
    a = run(sol, cost, cut, 0, None, None, None)
    b = run(a[3], a[4], moves - cut, cut, a[5], a[0], a[1])
    return one, (b[0], b[1], {k: a[2][k] + b[2][k] for k in KEYS}, b[3], b[4], b[5])


def _stack(arrays, dn, runs, dtypes):
    """runs: per case (one, two) of (best, best_cost, stats, sol, cost, temp)."""
    for pair in runs:
        for r in pair:
            got = [str(r[0].dtype), str(r[1].dtype), str(r[3].dtype), str(r[4].dtype), type(r[5]).__name__]
            assert dtypes == got, (dtypes, got)
    arrays[f"out/{dn}/sols"] = np.array([[[r[0], r[3]] for r in pair] for pair in runs])
    arrays[f"out/{dn}/costs"] = np.array([[[r[1], r[4]] for r in pair] for pair in runs])
    arrays[f"out/{dn}/scal"] = np.array([[[r[2][k] for k in KEYS] + [_bits(r[5])] for r in pair] for pair in runs],
                                        dtype=np.int64)


def _twin_cases():
    """geometric x max_retry x chain_base x offset"""
    return [dict(geometric=g, cool=0.97 if g else 2e-4, max_retry=mr, chain_base=cb, offset=off)
            for g, mr, cb, off in itertools.product((True, False), (0, 3), (0, BASE), (0, OFFSET))]


def _twins(tabs, start, reference, arrays, meta, dtypes):
    for dn, tb in tabs.items():
        cases = _twin_cases()
        runs = []
        for c in cases:
            key = f"start/{dn}/{c['chain_base']}"
            if key + "/sol" not in arrays:
                arrays[key + "/sol"], arrays[key + "/cost"] = start(tb, c["chain_base"])
            run = lambda s, k, n, b, t, best, bc: reference(tb, s, k, n, 0.05, c["cool"], INTERVAL, c["geometric"],
                                                            c["max_retry"], SEED, c["offset"], b, t, best, bc,
                                                            c["chain_base"])
            runs.append(_segments(run, arrays[key + "/sol"], arrays[key + "/cost"], MOVES, CUT))
        _stack(arrays, dn, runs, dtypes)
        meta["domains"][dn]["cases"] = cases
        meta["domains"][dn].update(P=P, moves=MOVES, cut=CUT, t0=0.05, interval=INTERVAL, seed=SEED)


_MT_ARRAYS = ("days", "hours", "minutes", "dur", "share", "member", "role_w", "blocked", "ordered", "cards",
              "share_b", "member_b")
_TWIN_DTYPES = ["int16", "float32", "int16", "float32", "float32"]


def meeting(out):
    from avenir_amd.optimize.domains import MeetingScheduleDomain
    from avenir_amd.optimize.ga_meeting import (ga_meeting_price, meeting_tables, sa_meeting_init,
                                                sa_meeting_reference)
    meta = {"dtypes": _TWIN_DTYPES, "domains": {}}
    arrays, tabs = {}, {}
    for dn, (M, Q, s) in {"smallest": (1, 3, 0), "reference": (10, 20, 3)}.items():   # tests/test_sa_meeting.py
        tb = tabs[dn] = meeting_tables(MeetingScheduleDomain.random_instance(M, Q, seed=s))
        for k in _MT_ARRAYS:
            arrays[f"dom/{dn}/{k}"] = tb[k]
        meta["domains"][dn] = {"M": tb["M"], "Q": tb["Q"], "L": tb["L"], "invalid": "inf"}

    def start(tb, base):
        sol = sa_meeting_init(tb, P, SEED, base)
        return sol, ga_meeting_price(tb, sol)

    _twins(tabs, start, sa_meeting_reference, arrays, meta, _TWIN_DTYPES)
    _save(out, "meeting.npz", meta, arrays)


def subset_ll(N, F, C):
    from avenir_amd.ops.random import philox4x32, u32_to_unit
    x = philox4x32(SEED_LL, 0, np.arange(N * F * C, dtype=np.uint64))[0]
    return (np.float32(-8.0) * u32_to_unit(x)).astype(np.float32).reshape(N, F, C)


def subset(out):
    from avenir_amd.optimize.domains import FeatureSubsetDomain
    from avenir_amd.optimize.ga_subset import (ga_subset_price, pack_masks, sa_subset_init, sa_subset_reference,
                                               subset_tables)
    meta = {"dtypes": _TWIN_DTYPES, "domains": {}}
    arrays, tabs = {}, {}
    shapes = {"smallest": (1, 1, 2, 0, 1), "short_tile": (300, 32, 16, 1, 32), "fixed_size": (517, 12, 3, 5, 5)}
    for dn, (N, F, C, lo, hi) in shapes.items():                                      # tests/test_sa_subset.py
        LL = subset_ll(N, F, C)
        rng = np.random.default_rng(77 + 100 * F + C)                                 # stored, not replayed
        prior = np.log(rng.dirichlet(np.full(C, 5.0))).astype(np.float32)
        labels = (LL[:, : max(1, F // 3), :].sum(1) + rng.normal(0, 2.0, (N, C))).argmax(1).astype(np.int32)
        labels[0] = C - 1
        arrays[f"dom/{dn}/log_prior"], arrays[f"dom/{dn}/labels"] = prior, labels
        tb = tabs[dn] = subset_tables(FeatureSubsetDomain(F, loglik=torch.from_numpy(LL), log_prior=torch.from_numpy(prior),
                                                          labels=torch.from_numpy(labels), min_size=lo, max_size=hi))
        assert tb is not None and tb["invalid"] == 1.0 and np.array_equal(tb["LL"], LL)
        meta["domains"][dn] = {"N": N, "F": F, "C": C, "min_size": lo, "max_size": hi, "invalid": 1.0,
                               "LL_sha256": hashlib.sha256(LL.tobytes()).hexdigest()}

    def start(tb, base):
        sol = sa_subset_init(tb, P, SEED, base)
        return sol, ga_subset_price(tb, pack_masks(sol))

    _twins(tabs, start, sa_subset_reference, arrays, meta, _TWIN_DTYPES)
    _save(out, "subset.npz", meta, arrays)


def _assignment(L, V, density, seed=3):
    """cost float32 [L, V], conflict bool [L, L] or None, as tests/test_optimize.py::_random_assignment"""
    from avenir_amd.optimize.domain import AssignmentDomain
    g = torch.Generator().manual_seed(seed)
    cost = torch.rand((L, V), generator=g) * 100
    conf = None
    if density:
        conf = torch.rand((L, L), generator=g) < density
        conf = conf | conf.T
    return AssignmentDomain(cost, conf, invalid_cost=1e3)


def _assign_start(d, n, seed):
    sol, ok = d.random(n, torch.Generator().manual_seed(seed))
    assert bool(ok.all())
    return sol.numpy().astype(np.int16), d.cost(sol).numpy().astype(np.float32)


def _same(a, b):
    return all(np.array_equal(a[i], b[i]) for i in (0, 1, 3, 4)) and a[2] == b[2] and _bits(a[5]) == _bits(b[5])


class _ExpShift:
    """np.exp moved ``ulps`` (+1, -1) units in the last place of its result."""

    def __init__(self, ulps):
        self.ulps, self.exp = ulps, np.exp

    def __enter__(self):
        if self.ulps:
            to = np.float32(np.inf if self.ulps > 0 else -np.inf)
            np.exp = lambda x, *a, **k: np.nextafter(self.exp(x, *a, **k), to)

    def __exit__(self, *exc):
        np.exp = self.exp


def assign(out):
    from avenir_amd.optimize.search import sa_assign_reference
    meta = {"dtypes": ["int64", "float32", "int64", "float32", "float32"], "domains": {}}
    arrays = {}
    # domain: L, V, conflict density, swap settings, t0, linear rate
    doms = {"L1_V2": (1, 2, 0.0, (False,), 30.0, 0.1), "L2_V2": (2, 2, 0.0, (True,), 30.0, 0.1),
            "L24_V10": (24, 10, 0.15, (True, False), 4.0, 0.02)}
    chains, moves, cut = 12, 60, 23
    for dn, (L, V, density, swaps, t0, rate) in doms.items():
        d = _assignment(L, V, density)
        cost = arrays[f"dom/{dn}/cost"] = d.cost_table.numpy().astype(np.float32)
        conf = None if d.conflict is None else d.conflict.numpy()
        if conf is not None:
            arrays[f"dom/{dn}/conflict"] = conf
        sol, cur = arrays[f"start/{dn}/0/sol"], arrays[f"start/{dn}/0/cost"] = _assign_start(d, chains, 3)
        cases, runs = [], []
        for swap, g, mr in itertools.product(swaps, (True, False), (0, 3)):
            for seed in range(11, 31):                     # until np.exp's last bit decides nothing
                run = lambda s, k, n, b, t, best, bc: sa_assign_reference(
                    cost, conf, swap, s, k, n, t0, 0.98 if g else rate, INTERVAL, g, mr, seed, OFFSET, b, t, best, bc, BASE)
                got = []
                for ulps in (0, 1, -1):
                    with _ExpShift(ulps):
                        got.append(_segments(run, sol, cur, moves, cut))
                if all(_same(got[0][i], x[i]) for x in got[1:] for i in (0, 1)):
                    break
            else:
                raise AssertionError(f"{dn}: no seed is free of last-bit decisions")
            assert seed == 11, "the docstring says one seed was tried per case"
            assert sum(got[0][0][2].values()) > 0
            cases.append(dict(swap=swap, geometric=g, cool=0.98 if g else rate, max_retry=mr, seed=seed))
            runs.append(got[0])
        _stack(arrays, dn, runs, meta["dtypes"])
        meta["domains"][dn] = dict(L=L, V=V, P=chains, moves=moves, cut=cut, t0=t0, interval=INTERVAL, offset=OFFSET,
                                   chain_base=BASE, cases=cases)
    _save(out, "assign.npz", meta, arrays)


def assign_gpu(out):
    from avenir_amd import _native
    dev = torch.device("cuda")
    meta = {"dtypes": ["int16", "float32", "int16", "float32"], "domains": {}}
    arrays = {}
    # domain: L, V, conflict density, swap, t0, linear rate
    doms = {"L1_V2": (1, 2, 0.0, False, 30.0, 0.1), "L2_V2": (2, 2, 0.0, True, 30.0, 0.1),
            "L40_V12": (40, 12, 0.1, True, 4.0, 0.02), "L512_V3": (512, 3, 0.0, False, 0.2, 1e-3)}
    moves, cut = 100, 37
    for dn, (L, V, density, swap, t0, rate) in doms.items():
        d = _assignment(L, V, density)
        cost = arrays[f"dom/{dn}/cost"] = d.cost_table.numpy().astype(np.float32)
        conf = None if d.conflict is None else d.conflict.numpy()
        if conf is not None:
            arrays[f"dom/{dn}/conflict"] = conf
        tcost = torch.from_numpy(cost).to(dev)
        tconf = None if conf is None else torch.from_numpy(conf).to(torch.uint8).to(dev)
        sol, cur = arrays[f"start/{dn}/0/sol"], arrays[f"start/{dn}/0/cost"] = _assign_start(d, 65, 3)

        def launches(n, c, cuts):
            s, k = torch.from_numpy(sol[:n]).to(dev), torch.from_numpy(cur[:n]).to(dev)
            best, bc = s.clone(), k.clone()
            temp, stats = t0, []
            for b, e in zip(cuts[:-1], cuts[1:]):
                st = torch.zeros(4, dtype=torch.long, device=dev)
                _native.C().sa_assign(tcost, tconf, swap, s, k, best, bc, e - b, t0, c["cool"], INTERVAL, c["geometric"],
                                      c["max_retry"], SEED, OFFSET, st, b, temp, BASE)
                stats.append(st.tolist())
                temp = float(np.array([stats[-1][3]], dtype=np.uint32).view(np.float32)[0])
            return [x.cpu().numpy() for x in (best, bc, s, k)], stats

        cases, sols, costs, scal = [], [], [], []
        for n, g, mr in itertools.product((1, 65), (True, False), (0, 3)):
            c = dict(chains=n, geometric=g, cool=0.98 if g else rate, max_retry=mr)
            one, s1 = launches(n, c, (0, moves))
            two, s2 = launches(n, c, (0, cut, moves))
            assert all(np.array_equal(a, b) for a, b in zip(one, two)), (dn, c)
            assert [a + b for a, b in zip(s2[0][:3], s2[1][:3])] == s1[0][:3] and s2[1][3] == s1[0][3], (dn, c)
            assert [str(x.dtype) for x in one] == meta["dtypes"] and sum(s1[0][:3]) > 0
            cases.append(c)
            pad = lambda x: np.concatenate([x, np.zeros((65 - n,) + x.shape[1:], dtype=x.dtype)])
            sols.append([pad(one[0] - sol[:n]), pad(one[2] - sol[:n])])
            costs.append([pad(one[1]), pad(one[3])])
            scal.append(s1 + s2)
        arrays[f"out/{dn}/sols"], arrays[f"out/{dn}/costs"] = np.array(sols), np.array(costs)
        arrays[f"out/{dn}/scal"] = np.array(scal, dtype=np.int64)
        meta["domains"][dn] = dict(L=L, V=V, swap=swap, moves=moves, cut=cut, t0=t0, interval=INTERVAL, seed=SEED,
                                   offset=OFFSET, chain_base=BASE, cases=cases)
    _save(out, "assign_gpu.npz", meta, arrays)


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else HERE
    os.makedirs(out, exist_ok=True)
    if "--gpu" in sys.argv:
        assign_gpu(out)
    else:
        meeting(out)
        subset(out)
        assign(out)
