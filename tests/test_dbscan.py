"""DBSCAN (models/dbscan.py, csrc/kernels/dbscan.hip): the numpy twin against sklearn on exactly
representable data, its edge cases, the squared threshold, and the device kernels bit for bit
against the twin (counts, core indices, labels) over every tile and template boundary."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch
from sklearn.cluster import DBSCAN as SkDBSCAN

from avenir_amd.models.dbscan import DBSCAN, dbscan_twin, eps_sq_threshold

SETTINGS = [("euclidean", 1.5), ("manhattan", 1.5), ("euclidean", 2.1)]


def lattice_case(seed):
    """Integer coordinates: every sum is exact and eps lies strictly between attainable distances."""
    rng = np.random.default_rng(seed)
    n, D = int(rng.integers(50, 701)), int(rng.integers(1, 5))
    side, ms = int(rng.integers(6, 31)), int(rng.integers(2, 8))
    return rng.integers(0, side, (n, D)).astype(np.float32), ms


def sk_fit(X, eps, ms, metric):
    m = SkDBSCAN(eps=eps, min_samples=ms, metric=metric, algorithm="brute").fit(X.astype(np.float64))
    return m.labels_.astype(np.int64), m.core_sample_indices_


def tie_points(X, eps, metric, labels, core_idx):
    """Border points with core neighbours in more than one cluster (fp64 distances: exact here)."""
    core = np.zeros(len(X), bool)
    core[core_idx] = True
    diff = X[:, None, :].astype(np.float64) - X[None, core, :]
    d = np.sqrt((diff ** 2).sum(-1)) if metric == "euclidean" else np.abs(diff).sum(-1)
    cl = labels[core]
    ties = 0
    for i in np.flatnonzero(~core & (labels >= 0)):
        ties += len(set(cl[d[i] <= eps])) > 1
    return ties


@functools.lru_cache(maxsize=None)
def lattice_reference(seed, k):
    metric, eps = SETTINGS[k]
    X, ms = lattice_case(seed)
    labels, core = sk_fit(X, eps, ms, metric)
    return X, ms, labels, core, tie_points(X, eps, metric, labels, core)


def check_twin(X, eps, ms, metric, labels, core):
    lab, cnt = dbscan_twin(X, eps, ms, metric)
    assert lab.dtype == np.int64 and cnt.dtype == np.int32
    assert np.array_equal(lab, labels)
    assert np.array_equal(np.flatnonzero(cnt >= ms), core)


# ---- CPU: the twin ------------------------------------------------------------------------------
def test_twin_equals_sklearn_on_lattices():
    ties = 0
    for seed in range(20):
        for k, (metric, eps) in enumerate(SETTINGS):
            X, ms, labels, core, t = lattice_reference(seed, k)
            check_twin(X, eps, ms, metric, labels, core)
            ties += t
    assert ties >= 1, "no border point with core neighbours in two clusters: the tie rule went untested"


def test_twin_edge_cases():
    one = np.zeros((1, 3), np.float32)
    lab, cnt = dbscan_twin(one, 0.5, 1)
    assert lab.tolist() == [0] and cnt.tolist() == [1]
    lab, cnt = dbscan_twin(one, 0.5, 2)
    assert lab.tolist() == [-1] and cnt.tolist() == [1]
    rng = np.random.default_rng(0)
    X = rng.integers(0, 3, (40, 2)).astype(np.float32)
    lab, cnt = dbscan_twin(X, 10.0, 41)                               # min_samples > n: all noise
    assert (lab == -1).all() and (cnt == 40).all()
    same = np.full((30, 4), 2.5, np.float32)                          # all rows identical
    lab, cnt = dbscan_twin(same, 0.0, 5)
    assert (lab == 0).all() and (cnt == 30).all()
    X = (rng.permutation(50) * 3).astype(np.float32)[:, None]         # min_samples = 1: every point core
    lab, cnt = dbscan_twin(X, 1.0, 1)
    assert (cnt == 1).all() and np.array_equal(lab, np.arange(50))
    base = rng.integers(0, 100, (12, 2)).astype(np.float32)           # eps = 0 with duplicated rows
    base = np.unique(base, axis=0)
    rep = rng.integers(1, 4, len(base))
    idx = rng.permutation(np.repeat(np.arange(len(base)), rep))
    lab, cnt = dbscan_twin(base[idx], 0.0, 2)
    assert np.array_equal(cnt, rep[idx])
    for g in range(len(base)):
        members = np.flatnonzero(idx == g)
        assert len(set(lab[members])) == 1 and (lab[members[0]] >= 0) == (rep[g] >= 2)
    ids = lab[lab >= 0]
    first = [np.flatnonzero(lab == c)[0] for c in range(ids.max() + 1)]
    assert first == sorted(first)                                     # numbered by smallest member


def test_twin_chain_root_is_smallest_member():
    rng = np.random.default_rng(1)
    pos = rng.permutation(300)
    X = pos.astype(np.float32)[:, None]                               # spacing 1, shuffled order
    lab, cnt = dbscan_twin(X, 1.0, 2)
    assert (lab == 0).all()
    assert np.array_equal(cnt, np.where((pos == 0) | (pos == 299), 2, 3))
    X2 = np.concatenate([X, X + 1000.0])                              # a second chain: opened later
    lab, _ = dbscan_twin(X2, 1.0, 2)
    assert (lab[:300] == 0).all() and (lab[300:] == 1).all()
    lab, _ = dbscan_twin(X2[::-1].copy(), 1.0, 2)                     # root = index of the smallest member
    assert (lab[:300] == 0).all() and (lab[300:] == 1).all()


def test_twin_rejects_bad_input():
    X = np.zeros((4, 2), np.float32)
    for bad in (X.astype(np.float64), np.zeros((0, 2), np.float32), np.zeros((4, 65), np.float32),
                np.zeros(4, np.float32), np.full((4, 2), np.nan, np.float32)):
        with pytest.raises(ValueError):
            dbscan_twin(bad, 0.5, 2)
    for eps, ms, metric in ((-1.0, 2, "euclidean"), (0.5, 0, "euclidean"), (0.5, 2, "cosine"), (np.inf, 2, "euclidean")):
        with pytest.raises(ValueError):
            dbscan_twin(X, eps, ms, metric)
    with pytest.raises(ValueError):
        DBSCAN(use_kernel=True).fit(torch.zeros(4, 2))                # no quiet fall-back


def test_eps_sq_threshold():
    rng = np.random.default_rng(2)
    eps = np.concatenate([10.0 ** rng.uniform(-30, 18, 900), rng.uniform(0, 4, 98), [0.0, 1.0]])
    inf = np.float32(np.inf)
    for e in eps:
        for e32 in (np.float32(e), e):                                # an fp32 value, and a double rounded to one
            t2 = eps_sq_threshold(e32)
            assert t2.dtype == np.float32 and np.isfinite(t2)
            assert np.sqrt(t2) <= np.float32(e32) < np.sqrt(np.nextafter(t2, inf))


def test_twin_chunking():
    X, ms = lattice_case(3)
    ref = dbscan_twin(X, 1.5, ms)
    rng = np.random.default_rng(4)
    G = (rng.normal(size=(500, 3)) + rng.integers(0, 3, (500, 1)) * 4).astype(np.float32)
    gref = dbscan_twin(G, 0.4, 5, "manhattan")
    for chunk in (1, 7, 64, 499, 500, 100000):
        for data, want, args in ((X, ref, (1.5, ms)), (G, gref, (0.4, 5, "manhattan"))):
            got = dbscan_twin(data, *args, chunk=chunk)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_model_on_cpu_is_the_twin():
    X, ms = lattice_case(5)
    m = DBSCAN(eps=1.5, min_samples=ms).fit(torch.from_numpy(X))
    lab, cnt = dbscan_twin(X, 1.5, ms)
    assert np.array_equal(m.labels_.numpy(), lab) and np.array_equal(m.counts_.numpy(), cnt)
    assert np.array_equal(m.core_sample_indices_.numpy(), np.flatnonzero(cnt >= ms))
    assert m.n_clusters_ == lab.max() + 1
    assert torch.equal(DBSCAN(eps=1.5, min_samples=ms).fit_predict(X), m.labels_)


# ---- GPU: the kernels against the twin, bit for bit ---------------------------------------------
NS = [1, 63, 64, 65, 255, 256, 257, 1000, 4099]
DS = [1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 64]


def lattice_wide(n, D, seed):
    """Integer lattice points that differ in at most three columns (the first, a middle one and the
    last, so padding and the last column both count) over a constant integer offset per column;
    about one point per five cells."""
    rng = np.random.default_rng(seed)
    cols = sorted({0, D // 2, D - 1})
    side = max(2, int(round((5 * n) ** (1.0 / len(cols)))))
    X = np.tile(rng.integers(-8, 9, D), (n, 1))
    X[:, cols] += rng.integers(0, side, (n, len(cols)))
    return X.astype(np.float32)


def blobs(n, D, metric, seed):
    """Gaussian blobs; eps one standard deviation of the in-blob distance below its mean, so that a
    sixth of a blob are neighbours, and min_samples about the mean count: core, border and noise."""
    rng = np.random.default_rng(seed)
    sigma = 0.37
    X = rng.normal(size=(4, D))[rng.integers(0, 4, n)] * 6 + sigma * rng.normal(size=(n, D))
    if metric == "euclidean":
        eps = sigma * max(np.sqrt(2 * D) - 1.0, 0.4)
    else:
        eps = sigma * max(1.128 * D - 0.85 * np.sqrt(D), 0.28)
    return X.astype(np.float32), float(eps), max(2, n // 40)


def check_device(X, eps, ms, metric, cuda, a_range=0, want=None):
    want = want or dbscan_twin(X, eps, ms, metric)
    m = DBSCAN(eps=eps, min_samples=ms, metric=metric, a_range=a_range).fit(torch.from_numpy(X).to(cuda))
    assert m.counts_.dtype == torch.int32 and m.labels_.dtype == torch.int64
    assert np.array_equal(m.counts_.cpu().numpy(), want[1])
    assert np.array_equal(m.core_sample_indices_.cpu().numpy(), np.flatnonzero(want[1] >= ms))
    assert np.array_equal(m.labels_.cpu().numpy(), want[0])
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["euclidean", "manhattan"])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("n", NS)
def test_kernels_lattice(cuda, n, D, metric):
    X = lattice_wide(n, D, 1000 * n + D)
    eps, ms = 1.5, 4
    labels, core = sk_fit(X, eps, ms, metric)
    check_twin(X, eps, ms, metric, labels, core)
    check_device(X, eps, ms, metric, cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["euclidean", "manhattan"])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("n", NS)
def test_kernels_blobs(cuda, n, D, metric):
    X, eps, ms = blobs(n, D, metric, 77 * n + D)
    check_device(X, eps, ms, metric, cuda)


def chains(n, seed):
    """Two interleaved 1-D chains at spacing 1, offset by 5 in a second coordinate, shuffled."""
    rng = np.random.default_rng(seed)
    X = np.stack([np.arange(n) // 2, (np.arange(n) % 2) * 5], 1).astype(np.float32)
    return X[rng.permutation(n)]


@pytest.mark.gpu
def test_kernels_deep_unions(cuda):
    rng = np.random.default_rng(6)
    X = rng.permutation(20000).astype(np.float32)[:, None]
    m = check_device(X, 1.0, 2, "euclidean", cuda)
    assert m.n_clusters_ == 1 and bool((m.labels_ == 0).all())
    X = chains(20000, 7)
    m = check_device(X, 1.0, 2, "euclidean", cuda)
    lab = m.labels_.cpu().numpy()
    assert m.n_clusters_ == 2
    first = int(X[0, 1])                                              # the chain of point 0 is cluster 0
    assert np.array_equal(lab, (X[:, 1].astype(int) != first).astype(np.int64))


@pytest.mark.gpu
def test_kernels_full_contention(cuda):
    rng = np.random.default_rng(8)
    X = rng.normal(size=(2048, 3)).astype(np.float32)
    for metric in ("euclidean", "manhattan"):
        m = check_device(X, 1000.0, 5, metric, cuda)
        assert bool((m.counts_ == 2048).all()) and m.n_clusters_ == 1


@pytest.mark.gpu
def test_kernels_border_ties_equal_sklearn(cuda):
    seed, k = max(((s, k) for s in range(20) for k in range(3)), key=lambda sk: lattice_reference(*sk)[4])
    X, ms, labels, core, ties = lattice_reference(seed, k)
    assert ties >= 1
    metric, eps = SETTINGS[k]
    m = check_device(X, eps, ms, metric, cuda)
    assert np.array_equal(m.labels_.cpu().numpy(), labels)
    assert np.array_equal(m.core_sample_indices_.cpu().numpy(), core)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [3, 40])
def test_kernels_grid_invariance(cuda, D):
    X, eps, ms = blobs(3000, D, "euclidean", 9)
    want = dbscan_twin(X, eps, ms)
    runs = [check_device(X, eps, ms, "euclidean", cuda, a_range=r, want=want) for r in (0, 0, 64, 1024)]
    for m in runs[1:]:
        assert torch.equal(m.labels_, runs[0].labels_) and torch.equal(m.counts_, runs[0].counts_)
    X = chains(5000, 10)
    if D > 3:
        X = np.concatenate([X, np.zeros((5000, D - 2), np.float32)], 1)
    want = dbscan_twin(X, 1.0, 2)
    for r in (0, 256, 2048):
        check_device(X, 1.0, 2, "euclidean", cuda, a_range=r, want=want)


@pytest.mark.gpu
def test_model_cuda_equals_cpu(cuda):
    X, eps, ms = blobs(1500, 6, "manhattan", 11)
    cpu = DBSCAN(eps, ms, "manhattan").fit(torch.from_numpy(X))
    for use_kernel in (None, True, False):
        dev = DBSCAN(eps, ms, "manhattan", use_kernel=use_kernel).fit(torch.from_numpy(X).to(cuda))
        assert dev.labels_.is_cuda and dev.n_clusters_ == cpu.n_clusters_
        assert torch.equal(dev.labels_.cpu(), cpu.labels_) and torch.equal(dev.counts_.cpu(), cpu.counts_)
        assert torch.equal(dev.core_sample_indices_.cpu(), cpu.core_sample_indices_)


@pytest.mark.gpu
def test_bindings_validate(cuda):
    from avenir_amd import _native
    C = _native.C()
    X = torch.zeros(8, 3, device=cuda)
    root = torch.zeros(8, dtype=torch.int32, device=cuda)
    for call in (lambda: C.dbscan_count(X.double(), 0, 1.0), lambda: C.dbscan_count(X.cpu(), 0, 1.0),
                 lambda: C.dbscan_count(X.t(), 0, 1.0), lambda: C.dbscan_count(torch.zeros(8, 65, device=cuda), 0, 1.0),
                 lambda: C.dbscan_count(X, 2, 1.0), lambda: C.dbscan_count(X, 0, -1.0),
                 lambda: C.dbscan_count(X, 0, float("nan")), lambda: C.dbscan_union(X, 0, 1.0, -1),
                 lambda: C.dbscan_border(X, X[:, :2].contiguous(), root, 0, 1.0),
                 lambda: C.dbscan_border(X, X, root[:4], 0, 1.0), lambda: C.dbscan_border(X, X, root.long(), 0, 1.0)):
        with pytest.raises(RuntimeError):
            call()
