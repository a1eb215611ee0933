"""The device Lloyd loops (kmeans_groups.hip), their host twin and ``KMeans.fit_many``.

CPU: the twin against the existing CPU path and on edge cases.  GPU: the kernel against the twin,
bit for bit (centroids, counts, iterations, converged flags; SSE and every history entry within the
reordering bound n 2^-52 of a sum of n non-negative doubles), launch-composition invariance, the
1024-thread class, the sklearn tolerance mode, the model and the job."""
import functools
import random

import numpy as np
import pytest
import torch

from avenir_amd.models import kmeans_groups as kg
from avenir_amd.models.cluster import KMeans
from avenir_amd.models.kmeans_groups import kmeans_fit_groups, kmeans_groups_twin


# ---------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kpp_rows():
    """The rows of test_data_parallel_jobs' ``kpp`` case: [(group, x, y)], values of 4 decimals."""
    rnd = random.Random(sum(map(ord, "kpp")))
    rows = []
    for _ in range(1200):
        g = rnd.randrange(7)
        c = rnd.randrange(3)
        rows.append((f"g{g}", f"{c * 4 + rnd.gauss(0, .3):.4f}", f"{c * 3 + rnd.gauss(0, .3):.4f}"))
    return rows


def _kpp_groups():
    by = {}
    for g, x, y in _kpp_rows():
        by.setdefault(g, []).append((float(x), float(y)))
    return [torch.tensor(by[g], dtype=torch.float32) for g in sorted(by)]


def _kpp_models(n=7):
    return [KMeans([2, 3, 4, 5], n_init=3, max_iter=10) for _ in range(n)]


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300) if a != b else 0.0


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def test_twin_matches_cpu_fit_on_kpp_data():
    Xs = _kpp_groups()
    assert len(Xs) == 7 and sum(X.shape[0] for X in Xs) == 1200
    models = _kpp_models()
    inits = KMeans.init_many(models, Xs)
    n_runs, max_dc, max_dsse = 0, 0.0, 0.0
    for km, X, C0 in zip(models, Xs, inits):
        km.fit(X, init_centroids=C0)
        assert len(km.runs) == 12
        for run, C in zip(km.runs, C0):
            Ct, cnt, sse, it, done, hist = kmeans_groups_twin(X.numpy(), C.numpy(), km.max_iter, km.tol, km.tol_mode)
            max_dc = max(max_dc, float(np.abs(Ct - run.centroids.numpy()).max()))
            max_dsse = max(max_dsse, _rel(sse, run.sse))
            assert it == run.iterations and done == run.converged
            assert np.array_equal(cnt, run.counts.numpy())
            assert np.array_equal(Ct, run.centroids.numpy())
            assert _rel(sse, run.sse) <= 1e-6
            assert len(hist) == it
            n_runs += 1
    print(f"twin vs fit: {n_runs} runs, max |dC| = {max_dc}, max rel dSSE = {max_dsse:.3g}")
    assert n_runs == 84


def test_fit_many_cpu_default_is_fit_and_use_kernel_is_the_twin():
    Xs = _kpp_groups()
    a, b, c = _kpp_models(), _kpp_models(), _kpp_models()
    inits = KMeans.init_many(a, Xs)
    out = KMeans.fit_many(a, Xs, inits)
    assert out is a
    for km, X, C0 in zip(b, Xs, inits):
        km.fit(X, init_centroids=C0)
    for ka, kb in zip(a, b):
        assert len(ka.runs) == len(kb.runs) == 12 and ka._shift is None
        for ra, rb in zip(ka.runs, kb.runs):
            assert (ra.k, ra.seed, ra.iterations, ra.converged) == (rb.k, rb.seed, rb.iterations, rb.converged)
            assert torch.equal(ra.centroids, rb.centroids) and torch.equal(ra.counts, rb.counts)
            assert ra.sse == rb.sse and ra.history == rb.history
        assert ka.knuckle_k() == kb.knuckle_k()
    KMeans.fit_many(c, Xs, inits, use_kernel=True)
    for kc, X, C0 in zip(c, Xs, inits):
        assert kc._shift is None and sorted(kc.best) == [2, 3, 4, 5]
        for run, C in zip(kc.runs, C0):
            Ct, cnt, sse, it, done, hist = kmeans_groups_twin(X.numpy(), C.numpy(), 10, kc.tol, "shift")
            assert np.array_equal(run.centroids.numpy(), Ct) and np.array_equal(run.counts.numpy(), cnt)
            assert (run.sse, run.iterations, run.converged, run.history) == (sse, it, done, hist)
        for k in kc.best:
            assert kc.best[k].sse == min(r.sse for r in kc.runs if r.k == k)
        assert kc.predict(X).shape[0] == X.shape[0]
    # without inits they come from init_many: the same fit
    d = _kpp_models(1)
    KMeans.fit_many(d, Xs[:1])
    assert all(torch.equal(r1.centroids, r2.centroids) for r1, r2 in zip(d[0].runs, a[0].runs))


def test_fit_many_env_switch_forces_the_per_model_path(monkeypatch):
    Xs = _kpp_groups()[:2]
    calls = []
    monkeypatch.setattr(kg, "kmeans_fit_groups", lambda *a, **k: calls.append(1) or [])
    monkeypatch.setenv("AVMI_KMEANS_GROUPS", "0")
    ms = KMeans.fit_many(_kpp_models(2), Xs, use_kernel=True)
    assert not calls and all(len(m.runs) == 12 for m in ms)


EDGE = {
    # name: (X, C0)
    "empty": (np.array([[0, 0], [0.5, 0.25], [1, 0], [0.25, 1]], np.float32),
              np.array([[0, 0], [1e6, 1e6]], np.float32)),
    "zeros": (np.zeros((10, 2), np.float32), np.array([[0, 0], [1, 1]], np.float32)),
    "n_eq_k": (np.array([[0, 0], [3, 1], [-2, 5], [7, 7]], np.float32),
               np.array([[0, 0], [3, 1], [-2, 5], [7, 7]], np.float32)),
    "dups": (np.array([[1, 1]] * 4 + [[2, 2]] * 2, np.float32), np.array([[1, 1], [1, 1], [2, 2], [2, 2]], np.float32)),
}


def test_twin_edge_cases():
    X, C0 = EDGE["empty"]
    C, cnt, sse, it, done, hist = kmeans_groups_twin(X, C0, 10, 1e-4)
    assert cnt.tolist() == [4, 0] and np.array_equal(C[1], C0[1]) and done
    assert np.array_equal(C[0], X.mean(0))
    # max_iter = 0: the inits with their SSE and counts
    C, cnt, sse, it, done, hist = kmeans_groups_twin(X, C0, 0, 1e-4)
    assert np.array_equal(C, C0) and it == 0 and not done and hist == []
    assert cnt.tolist() == [4, 0] and sse == float((X.astype(np.float64) ** 2).sum())
    X, C0 = EDGE["zeros"]
    C, cnt, sse, it, done, hist = kmeans_groups_twin(X, C0, 10, 1e-4)
    assert cnt.tolist() == [10, 0] and sse == 0.0 and np.array_equal(C, C0) and done and it == 1
    X, C0 = EDGE["n_eq_k"]
    C, cnt, sse, it, done, hist = kmeans_groups_twin(X, C0, 10, 1e-4)
    assert it == 1 and done and sse == 0.0 and cnt.tolist() == [1, 1, 1, 1] and np.array_equal(C, C0)
    X, C0 = EDGE["dups"]
    C, cnt, sse, it, done, hist = kmeans_groups_twin(X, C0, 10, 1e-4)
    assert cnt.tolist() == [4, 0, 2, 0] and sse == 0.0
    for bad in (np.inf, -np.inf, np.nan):
        Xb = EDGE["n_eq_k"][0].copy()
        Xb[2, 1] = bad
        with pytest.raises(ValueError):
            kmeans_groups_twin(Xb, EDGE["n_eq_k"][1], 10, 1e-4)
    with pytest.raises(ValueError):
        kmeans_fit_groups([torch.from_numpy(Xb)], [0], [torch.from_numpy(EDGE["n_eq_k"][1])], 10, 1e-4, device="cpu")


# ---------------------------------------------------------------------------------------------
# GPU: kernel against twin
# ---------------------------------------------------------------------------------------------
SIZES = [1, 63, 64, 65, 1000, 4097]
MAX_ITER = 8


@functools.lru_cache(maxsize=None)
def _case(D):
    """Groups, runs and inits of the bit-exactness case at D, with the twin's results (computed
    once, shared by the tests).  Group g is on a coarse grid (multiples of 2^-8, |x| < 2^7) when g
    is even, raw randn * 10^U(-3, 3) per element when odd."""
    rng = np.random.default_rng(100 + D)
    Xs, wide = [], []
    for g, n in enumerate(SIZES):
        if g % 2 == 0:
            X = rng.integers(-(1 << 15) + 1, 1 << 15, size=(n, D)).astype(np.float32) / np.float32(256)
        else:
            X = (rng.standard_normal((n, D)) * 10.0 ** rng.uniform(-3, 3, size=(n, D))).astype(np.float32)
            wide.append(g)
        Xs.append(X)
    run_group, inits = [], []
    for g, X in enumerate(Xs):
        for k in range(1, 6):
            for _ in range(3):
                run_group.append(g)
                inits.append(X[rng.integers(0, X.shape[0], size=k)].copy())
    if D == 16:   # one k = 64 run on the largest group
        run_group.append(len(SIZES) - 1)
        inits.append(Xs[-1][rng.choice(Xs[-1].shape[0], size=64, replace=False)].copy())
    if D == 2:    # the twin's edge cases as groups of their own
        for name in ("empty", "zeros", "n_eq_k", "dups"):
            X, C0 = EDGE[name]
            Xs.append(X)
            run_group.append(len(Xs) - 1)
            inits.append(C0)
    twin = [kmeans_groups_twin(Xs[g], C0, MAX_ITER, 1e-4) for g, C0 in zip(run_group, inits)]
    return Xs, run_group, inits, twin, wide


def _fit_gpu(Xs, run_group, inits, max_iter=MAX_ITER, tol=1e-4, mode="shift", effs=None):
    return kmeans_fit_groups([torch.from_numpy(X) for X in Xs], run_group, [torch.from_numpy(C) for C in inits],
                             max_iter, tol, mode, effs, "cuda")


def _assert_equals_twin(res, twin, ns):
    """ns[r]: rows of run r's group (the SSE reordering bound n 2^-52, relative)."""
    worst = 0.0
    for r, (got, (C, cnt, sse, it, done, hist)) in enumerate(zip(res, twin)):
        assert got.iterations == it and got.converged == done, r
        assert np.array_equal(got.counts.numpy(), cnt), r
        assert np.array_equal(got.centroids.cpu().numpy(), C), r
        bound = ns[r] * 2.0 ** -52
        assert len(got.history) == len(hist) == it
        for a, b in zip([got.sse] + got.history, [sse] + hist):
            worst = max(worst, _rel(a, b) / bound)
            assert _rel(a, b) <= bound, (r, a, b)
    print(f"{len(res)} runs equal the twin; worst SSE difference = {worst:.3g} of the bound")


@pytest.mark.gpu
@pytest.mark.parametrize("D", [2, 3, 16])
def test_kernel_equals_twin(cuda, D):
    Xs, run_group, inits, twin, _ = _case(D)
    res = _fit_gpu(Xs, run_group, inits)
    assert len(res) == len(twin) == 90 + (1 if D == 16 else 0) + (4 if D == 2 else 0)
    _assert_equals_twin(res, twin, [Xs[g].shape[0] for g in run_group])
    if D == 2:    # the edge cases did what the twin's tests say
        emp, zer, nk, dup = res[-4:]
        assert emp.counts.tolist() == [4, 0] and zer.counts.tolist() == [10, 0] and zer.sse == 0.0
        assert nk.iterations == 1 and nk.converged and nk.sse == 0.0 and dup.counts.tolist() == [4, 0, 2, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("D", [2, 3, 16])
def test_launch_composition_invariance(cuda, D):
    Xs, run_group, inits, _, wide = _case(D)
    rng = np.random.default_rng(7)
    fill = [rng.standard_normal((int(n), D)).astype(np.float32) for n in rng.integers(20, 700, size=200)]
    fill_inits = [X[:3].copy() for X in fill]
    sel = [r for r, g in enumerate(run_group) if g in wide]
    gmap = {g: i for i, g in enumerate(wide)}
    together = _fit_gpu(fill[:100] + [Xs[g] for g in wide] + fill[100:],
                        list(range(100)) + [100 + gmap[run_group[r]] for r in sel]
                        + [100 + len(wide) + i for i in range(100)],
                        fill_inits[:100] + [inits[r] for r in sel] + fill_inits[100:])[100:100 + len(sel)]
    alone = []
    for g in wide:
        rs = [r for r in sel if run_group[r] == g]
        alone += _fit_gpu([Xs[g]], [0] * len(rs), [inits[r] for r in rs])
    assert len(alone) == len(together) == len(sel)
    for a, b in zip(alone, together):
        assert torch.equal(a.centroids, b.centroids) and torch.equal(a.counts, b.counts)
        assert (a.sse, a.iterations, a.converged, a.history) == (b.sse, b.iterations, b.converged, b.history)


@pytest.mark.gpu
@pytest.mark.parametrize("n,D", [(70_000, 2), (20_000, 16)])
def test_streamed_group_equals_twin(cuda, n, D):
    rng = np.random.default_rng(n + D)
    cen = rng.standard_normal((4, D)).astype(np.float32) * 4
    X = (cen[rng.integers(0, 4, size=n)] + rng.standard_normal((n, D))).astype(np.float32)
    inits = [X[rng.choice(n, size=k, replace=False)].copy() for k in (2, 3, 4) for _ in range(3)]
    twin = [kmeans_groups_twin(X, C0, 10, 1e-4) for C0 in inits]
    res = _fit_gpu([X], [0] * 9, inits, max_iter=10)
    _assert_equals_twin(res, twin, [n] * 9)


@pytest.mark.gpu
@pytest.mark.parametrize("n,D,k", [(300, 20, 7), (300, 40, 64), (9000, 64, 5)])
def test_wide_rows_equal_twin(cuda, n, D, k):
    """D padded to 32 and 64; k = 64 at Dp = 64 is the largest LDS image (one replica, above
    64 KiB); 9,000 x 64 is the 1024-thread class without the row prefetch."""
    rng = np.random.default_rng(n + D + k)
    X = (rng.standard_normal((n, D)) * 10.0 ** rng.uniform(-2, 2, size=(n, D))).astype(np.float32)
    inits = [X[rng.choice(n, size=k, replace=False)].copy() for _ in range(2)]
    twin = [kmeans_groups_twin(X, C0, 5, 1e-4) for C0 in inits]
    _assert_equals_twin(_fit_gpu([X], [0, 0], inits, max_iter=5), twin, [n, n])


@pytest.mark.gpu
def test_sklearn_tolerance_mode(cuda):
    rng = np.random.default_rng(5)
    X = (rng.standard_normal((1000, 4)) + 3 * rng.integers(0, 3, size=(1000, 1))).astype(np.float32)
    inits = [X[rng.choice(1000, size=k, replace=False)].copy() for k in (2, 3, 4, 5)]
    eff = float(X.astype(np.float64).var(0).mean()) * 1e-3
    twin = [kmeans_groups_twin(X, C0, 30, 1e-3, "sklearn", eff) for C0 in inits]
    shift = [kmeans_groups_twin(X, C0, 30, 1e-3, "shift") for C0 in inits]
    assert [t[3] for t in twin] != [t[3] for t in shift]      # the mode matters on this data
    res = _fit_gpu([X], [0] * 4, inits, max_iter=30, tol=1e-3, mode="sklearn", effs=[eff] * 4)
    for got, (C, cnt, sse, it, done, hist) in zip(res, twin):
        assert got.iterations == it and got.converged == done
        assert np.array_equal(got.centroids.cpu().numpy(), C)
    # the model computes the same threshold from the data
    km = KMeans([3], n_init=1, max_iter=30, tol=1e-3, tol_mode="sklearn")
    KMeans.fit_many([km], [torch.from_numpy(X).cuda()], [[torch.from_numpy(inits[1]).cuda()]])
    assert km.runs[0].iterations == twin[1][3] and km._tol_eff == pytest.approx(eff, rel=1e-6)


# ---------------------------------------------------------------------------------------------
# GPU: model and job
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fit_many_model_level(cuda, monkeypatch):
    Xs = _kpp_groups()
    calls = []
    real = kg.kmeans_fit_groups
    monkeypatch.setattr(kg, "kmeans_fit_groups", lambda *a, **k: calls.append(1) or real(*a, **k))
    gm, cm = _kpp_models(), _kpp_models()
    Xd = [X.to(cuda) for X in Xs]
    inits = KMeans.init_many(gm, Xd)
    KMeans.fit_many(gm, Xd, inits)
    assert len(calls) == 1
    for kg_, kc, X, C0 in zip(gm, cm, Xs, inits):
        kc.fit(X, init_centroids=[C.cpu() for C in C0])
        assert len(kg_.runs) == len(kc.runs) == 12 and kg_._shift is None
        for a, b in zip(kg_.runs, kc.runs):
            assert a.iterations == b.iterations and torch.equal(a.counts.cpu(), b.counts)
            assert float((a.centroids.cpu() - b.centroids).abs().max()) <= 1e-6
            assert _rel(a.sse, b.sse) <= 1e-6
        assert kg_.knuckle_k() == kc.knuckle_k()
        assert kg_.predict(X.to(cuda)).shape[0] == X.shape[0]


@pytest.mark.gpu
def test_job_uses_the_batched_path(cuda, tmp_path, monkeypatch):
    from avenir_amd.cli import main
    data = tmp_path / "km.csv"
    data.write_text("".join(f"{g},{x},{y}\n" for g, x, y in _kpp_rows()))
    conf = tmp_path / "job.conf"
    outs = {}
    calls = []
    real = kg.kmeans_fit_groups
    monkeypatch.setattr(kg, "kmeans_fit_groups", lambda *a, **k: calls.append(1) or real(*a, **k))
    for dev in ("cuda", "cpu"):
        conf.write_text("kMeansPlusPlusCluster {\n  field.delim.in = \",\"\n  id.fieldOrdinals = [0]\n"
                        "  num.clusters = [2,3,4]\n  num.iter = 10\n  num.clustGroup = 3\n"
                        f"  cluster.outputPath = \"{tmp_path / ('cent_' + dev)}\"\n}}\n")
        before = len(calls)
        assert main(["kMeansPlusPlusCluster", "-i", str(data), "-o", str(tmp_path / dev), "-c", str(conf),
                     "--device", dev]) == 0
        assert len(calls) - before == (1 if dev == "cuda" else 0)

        def lines(p):
            return [l for f in sorted(p.iterdir()) if f.is_file() for l in f.read_text().splitlines() if l.strip()] \
                if p.is_dir() else [l for l in p.read_text().splitlines() if l.strip()]
        outs[dev] = (lines(tmp_path / dev), lines(tmp_path / ("cent_" + dev)))
    kn = {d: [l for l in outs[d][0] if "knuckle" in l] for d in outs}
    assert kn["cuda"] == kn["cpu"] and len(kn["cpu"]) == 7
    assert len(outs["cuda"][0]) == len(outs["cpu"][0]) == 7 * 4
    assert len(outs["cuda"][1]) == len(outs["cpu"][1]) == 7 * (2 + 3 + 4)


@pytest.mark.gpu
def test_binding_validation(cuda):
    from avenir_amd import _native
    C = _native.C()
    X = torch.zeros((100, 2), device=cuda)
    groups = torch.tensor([[0, 100]])
    thr = torch.zeros(1, dtype=torch.float64)

    def call(X=X, groups=groups, runs=torch.tensor([[0, 2, 0]]), C0=None, thr=thr, D=None, k=2):
        C0 = torch.zeros((k, X.shape[1]), device=cuda) if C0 is None else C0
        return C.kmeans_fit_groups(X, groups, runs, C0, thr, X.shape[1] if D is None else D, 5, 0)

    assert len(call()) == 7
    with pytest.raises(RuntimeError, match=r"k must be in \[1, 64\]"):
        call(runs=torch.tensor([[0, 65, 0]]), k=65)
    with pytest.raises(RuntimeError, match="padded to 2/4/8/16/32/64"):
        call(X=torch.zeros((100, 128), device=cuda))
    with pytest.raises(RuntimeError, match="past the group table"):
        call(runs=torch.tensor([[1, 2, 0]]))
    with pytest.raises(RuntimeError, match="past the centroid table"):
        call(runs=torch.tensor([[0, 2, 1]]))
    with pytest.raises(RuntimeError, match="outside X"):
        call(groups=torch.tensor([[1, 100]]))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        call(C0=torch.zeros((2, 2)))
    # the wrapper refuses D > 64 and reports non-finite data of any group
    with pytest.raises(ValueError):
        kmeans_fit_groups([torch.zeros((10, 65))], [0], [torch.zeros((2, 65))], 5, 1e-4, device="cuda")
    Xb = torch.ones((300, 3))
    Xb[299, 2] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        kmeans_fit_groups([torch.ones((5, 3)), Xb], [0, 1], [torch.zeros((1, 3)), torch.zeros((2, 3))], 5, 1e-4,
                          device="cuda")
