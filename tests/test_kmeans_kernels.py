"""The three k-means Lloyd-pass kernels (kmeans_score_kernel, kmeans_mfma_kernel, kmeans_step_kernel)
on data where the answer is exact, in every arithmetic mode, plus the offset-data fit and the
batched k-means++ seeding.  The cases and their references live in tests/_kmeans_cases.py.

A. integer battery: bit-exact assign (lowest index on ties) / counts / sums / sse at every dispatch
   arm of km_variant, n in {1, 63, 64, 65, 257} and one n at which every wave rotates >= 3 tiles.
B. every AVMI_KMEANS_* mode in a fresh child process (the knobs are read once per process).
C. workgroup partial sums are exact fp32 sums of the fp32 data in every mode.
D. a GPU fit of data with a large common offset equals the fp64 Lloyd iteration.
E. batched (padded) k-means++ seeding equals per-group seeding.
"""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

import _kmeans_cases as K
from avenir_amd.models.cluster import KMeans, kmeans_step

HELPER = os.path.abspath(K.__file__)


# ---------------------------------------------------------------------------------------------
# A
@pytest.mark.gpu
@pytest.mark.parametrize("shape", K.SCORE_SHAPES, ids=str)
def test_exact_integers_score_kernel(cuda, shape):
    fails = K.battery(shape, cuda)
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", K.MFMA_SHAPES + K.MULTI_RUNS, ids=str)
def test_exact_integers_mfma_kernel(cuda, shape):
    fails = K.battery(shape, cuda)
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", K.LDS_SHAPES, ids=str)
def test_exact_integers_lds_kernel(cuda, shape):
    fails = K.battery(shape, cuda, lds=True)
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,lds", [((16, 16), False), ((32, 16), False), ((4, 17), False),   # score kernel
                                       ((16, 40), False), ((16, [1, 3, 16, 7]), False),          # MFMA kernel
                                       ((64, 70), True)], ids=str)                               # LDS kernel
def test_exact_integers_three_tiles_per_wave(cuda, shape, lds):
    """n = 64 (3 * 1024 + 37) + 17: on the launched grid (read from the partials) every wave walks at
    least three tiles, so both register buffers, the clamped prefetch past the last tile, the
    xnext prefetch and the grid-stride loop run, and the last tile is ragged."""
    fails = K.battery_big(shape, cuda, lds=lds)
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,lds", [((16, 16), False), ((4, 3), False), ((16, 40), False), ((16, 300), True)],
                         ids=str)
def test_identical_centroids_lower_index_takes_every_row(cuda, shape, lds):
    fails = K.battery(shape, cuda, lds=lds, dup=True)
    assert not fails, "\n".join(fails)
    D, k = shape
    X, Cs = K.int_data(257, D, [k], seed=3, dup=True)
    got, _ = K.run_step(X.to(cuda), [Cs[0].to(cuda)])
    sums, counts, _, assign = got[0]
    assert not bool((assign == k - 1).any()) and float(counts[k - 1]) == 0.0 and not bool(sums[k - 1].any())


# ---------------------------------------------------------------------------------------------
# B
MODES = {"default": {}, "f32": {"AVMI_KMEANS_MFMA": "f32"}, "bf16x6": {"AVMI_KMEANS_MFMA": "bf16x6"},
         "f32_nbuf3": {"AVMI_KMEANS_MFMA": "f32", "AVMI_KMEANS_NBUF": "3"}, "valu": {"AVMI_KMEANS_SCORE": "valu"}}
# one child (interpreter start, torch import, 77 launches with their references) measured on an
# MI355X: 3.2-3.3 s in every mode; about 3x headroom
CHILD_TIMEOUT = 12.0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(MODES))
def test_every_mode_in_a_fresh_process(cuda, mode):
    """Battery A on the score-kernel shapes (small n and the three-tile n) and C, with the mode's
    AVMI_KMEANS_* knobs set for a fresh Python process; one child at a time, no retry."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("AVMI_KMEANS_")}
    env.update(MODES[mode])
    p = subprocess.run([sys.executable, HELPER], env=env, timeout=CHILD_TIMEOUT, capture_output=True, text=True)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    verdict = json.loads(lines[-1]) if lines else None
    assert p.returncode == 0 and verdict is not None and verdict["ok"], \
        f"mode {mode}: exit {p.returncode}\n{json.dumps(verdict, indent=1)}\n{p.stderr[-2000:]}"
    assert verdict["mode"] == MODES[mode]


# ---------------------------------------------------------------------------------------------
# C
@pytest.mark.gpu
@pytest.mark.parametrize("scale", K.SUMS_SCALES, ids=["x1", "x2^13"])
@pytest.mark.parametrize("kind,D", [("score", 8), ("score", 16), ("score", 32), ("mfma", 8), ("mfma", 16),
                                    ("mfma", 32), ("lds", 16)])
def test_partial_sums_are_fp32_exact(cuda, kind, D, scale):
    """4096 rows, 16 clusters, 20-bit coordinates in [1, 2) (and x 2^13): every workgroup adds at
    most 16 rows per cluster, so its sums fit 24 bits and the reduced sums must EQUAL the fp64
    index_add.  The split-bf16 modes (D = 16 / 32) need all three bf16 terms of a row in the
    partial-sum operand for that: two terms keep 16-17 of the 20 bits."""
    fails = K.check_sums(D, scale, cuda, kind)
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------
# D
BLOB_N = 20_000


def _blobs(D: int, shift: float):
    g = torch.Generator().manual_seed(100 + D)
    lab = torch.randint(0, 4, (BLOB_N,), generator=g)
    centres = (torch.arange(4).double() * 8.0).view(4, 1).expand(4, D)
    X = (centres[lab] + torch.randn((BLOB_N, D), generator=g).double() + shift).float()
    init = (centres + 0.5 * torch.randn((4, D), generator=g).double() + shift).float()
    return X, init, lab, centres + shift


def _lloyd64(X: torch.Tensor, C0: torch.Tensor, max_iter: int, tol: float):
    """fp64 Lloyd iteration with direct distances: (centroids, assignment, sse) at convergence."""
    Xd, C = X.double(), C0.double()
    k = C.shape[0]
    for _ in range(max_iter):
        a = (torch.cdist(Xd, C) ** 2).argmin(1)
        cnt = torch.bincount(a, minlength=k).double().view(-1, 1)
        new = torch.where(cnt > 0, torch.zeros_like(C).index_add_(0, a, Xd) / cnt.clamp_min(1), C)
        move = float((new - C).norm(dim=1).max())
        C = new
        if move <= tol:
            break
    d2 = torch.cdist(Xd, C) ** 2
    a = d2.argmin(1)
    return C, a, float(d2.gather(1, a.view(-1, 1)).sum())


_LLOYD = {}


def _offset_case(D: int, shift: float):
    if (D, shift) not in _LLOYD:
        X, init, lab, centres = _blobs(D, shift)
        _LLOYD[(D, shift)] = (X, init, lab, centres, _lloyd64(X, init, 50, 1e-4))
    return _LLOYD[(D, shift)]


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0.0, 1e3, 1e4])
@pytest.mark.parametrize("D", [6, 16])
def test_offset_data_fit_equals_fp64_lloyd(cuda, D, shift):
    """Four unit-normal blobs 8 apart in every dimension plus a common feature offset.  Un-centred,
    the fp32 ||c||^2 - 2 x.c scores (magnitude ~D offset^2) round by more than the blob separation
    at offset 1e4 (1e3 at D = 16 in the split-bf16 default); KMeans.fit translates by the feature
    mean first."""
    X, init, lab, centres, (C64, a64, sse64) = _offset_case(D, shift)
    # reference alone: the fp64 Lloyd recovers the four blobs
    assert torch.equal(a64, lab)
    assert float((C64 - centres).abs().max()) < 0.1
    km = KMeans(4, max_iter=50).fit(X.to(cuda), init_centroids=[init.to(cuda)])
    run = km.best[4]
    print(f"D {D} shift {shift:g}: counts {run.counts.tolist()} vs {torch.bincount(a64, minlength=4).tolist()}, "
          f"max centroid error {float((run.centroids.cpu().double() - C64).abs().max()):.3g}, "
          f"sse {run.sse!r} vs {sse64!r}")
    assert torch.equal(run.counts.cpu().long(), torch.bincount(a64, minlength=4))
    bound = math.ceil(BLOB_N / 256) * 2.0 ** -24 * float(X.abs().max())
    assert float((run.centroids.cpu().double() - C64).abs().max()) <= bound
    assert run.sse == pytest.approx(sse64, rel=1e-3)
    assert torch.equal(km.predict(X.to(cuda)).cpu().long(), a64)


@pytest.mark.gpu
def test_step_kernel_oracle_tie_allowance_on_centred_data(cuda):
    """The kernel oracle's tie allowance 1e-5 (1 + ||x||^2 + max ||c||^2) of
    test_kmeans_step_kernel_matches_oracle, applied to offset data AFTER the fit's centring: the
    allowance is then that of the centred magnitudes and no longer grows with the offset."""
    for D, k in ((16, 16), (8, 20), (16, 40), (16, 300)):
        g = torch.Generator().manual_seed(D + k)
        X = (torch.randn((20_000, D), generator=g).double() + 1e4).float()
        C = X[torch.randperm(X.shape[0], generator=g)[:k]] + 0.25
        mean = X.double().mean(0).float()
        Xc, Cc = X - mean, C - mean
        sums, counts, sse, assign = kmeans_step(Xc.to(cuda), [Cc.to(cuda)], True)[0]
        d2 = torch.cdist(Xc.double(), Cc.double()) ** 2
        ref_a, a = d2.argmin(1), assign.cpu().long()
        gap = (d2.gather(1, a.view(-1, 1)) - d2.gather(1, ref_a.view(-1, 1))).view(-1)
        tol = 1e-5 * (1 + (Xc.double() ** 2).sum(1) + (Cc.double() ** 2).sum(1).max())
        assert float(tol.max()) < 1e-2                      # centred: not the 1e-5 D 1e8 of the raw data
        assert bool(((a == ref_a) | (gap.abs() <= tol)).all())
        ref_sums = torch.zeros((k, D), dtype=torch.float64).index_add_(0, a, Xc.double())
        assert torch.allclose(sums.cpu(), ref_sums, atol=1e-2, rtol=1e-4)
        assert torch.equal(counts.cpu().round().long(), torch.bincount(a, minlength=k))
        assert float(sse) == pytest.approx(float(d2.gather(1, a.view(-1, 1)).sum()), rel=1e-4)


# ---------------------------------------------------------------------------------------------
# E
def _seed_groups(dev):
    g = torch.Generator().manual_seed(9)
    sizes, ks = [5, 40, 41, 300], [3, 7, 4, 5]             # one (D, L) key: k 3..7 all draw L = 3 candidates
    Xs = [torch.randn((m, 3), generator=g).to(dev) for m in sizes]
    Xs += [torch.full((12, 3), 2.5).to(dev),               # all rows identical: zero potential
           torch.randn((4, 3), generator=g).to(dev),        # fewer rows than k
           torch.randn((1, 3), generator=g).to(dev)]        # a single row
    ks += [4, 6, 3]
    return Xs, [KMeans(k, n_init=2, seed=11 + i) for i, k in enumerate(ks)]


def _check_seeding(dev):
    Xs, models = _seed_groups(dev)
    batched = KMeans.init_many(models, Xs)
    for X, km, Cs in zip(Xs, models, batched):
        own = km._init_centroids_all(X, km.run_specs())
        assert len(Cs) == len(own) == km.n_init
        for C, Co in zip(Cs, own):
            assert C.shape == (km.ks[0], 3)
            assert torch.equal(C, Co)
            # every centre is a row of its own group (never a zero-padded row of the batch)
            assert bool((C.unsqueeze(1) == X.float().unsqueeze(0)).all(2).any(1).all())


def test_seeding_batch_equals_per_group_seeding():
    _check_seeding(torch.device("cpu"))


@pytest.mark.gpu
def test_seeding_batch_equals_per_group_seeding_gpu(cuda):
    _check_seeding(cuda)
