"""The isolation forest kernels (csrc/kernels/iforest.hip) against the numpy twin (models/iforest.py):
the build kernel bit for bit in feat / thr / size, the score kernel bit for bit in the path length,
the bindings' refusals, and the model and the verb on cuda against cpu.  Every expected value comes
from the twin."""
from __future__ import annotations

from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import torch

from avenir_amd.models import iforest as IF
from avenir_amd.models.outlier import IsolationForest

pytestmark = pytest.mark.gpu
BIG_BASE = (1 << 32) + 5


@lru_cache(maxsize=None)
def rows(D, n=5000):
    return np.random.default_rng(100 + D).normal(size=(n, D)).astype(np.float32)


@lru_cache(maxsize=None)
def twin(D, n, T, psi, seed, base):
    return IF.iforest_build_twin(rows(D)[:n], T, psi, seed, base)


def C():
    from avenir_amd import _native
    return _native.C()


def kernel_build(X, T, psi, seed, base, cuda):
    return tuple(t.cpu().numpy() for t in C().iforest_build(torch.from_numpy(X).to(cuda), T, psi, seed, base))


def same(got, want):
    for a, b, name in zip(got, want, ("feat", "thr", "size")):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), name


# every psi with every D; n = psi and n = 5000, T, and tree_base rotate through the grid
PSIS, DS = [1, 2, 5, 63, 64, 65, 256, 257, 1000], [1, 3, 33, 64]
GRID = [(psi, D, (psi if (i + j) % 2 else 5000), (1, 7, 130)[(i + 2 * j) % 3] if psi < 1000 else (1, 7)[j % 2],
         (0, BIG_BASE)[(i + j // 2) % 2]) for i, psi in enumerate(PSIS) for j, D in enumerate(DS)]


@pytest.mark.parametrize("psi,D,n,T,base", GRID)
def test_build_kernel_equals_twin(cuda, psi, D, n, T, base):
    same(kernel_build(rows(D)[:n], T, psi, 17, base, cuda), twin(D, n, T, psi, 17, base))


def test_build_kernel_many_trees_large_sample(cuda):
    same(kernel_build(rows(3), 130, 1000, 5, BIG_BASE, cuda), twin(3, 5000, 130, 1000, 5, BIG_BASE))   # LDS tile
    same(kernel_build(rows(64), 130, 257, 5, 0, cuda), twin(64, 5000, 130, 257, 5, 0))                   # global rows


def special_inputs():
    rng = np.random.default_rng(11)
    huge = rng.normal(size=(300, 3)).astype(np.float32)
    huge[::3], huge[1::3] = np.float32(3e38), np.float32(-3e38)
    const_col = rng.normal(size=(300, 33)).astype(np.float32)
    const_col[:, 1] = 2.5
    return {"constant": np.ones((300, 2), np.float32),
            "lattice": rng.integers(0, 4, size=(600, 3)).astype(np.float32),
            "constant_column": const_col, "huge": huge,
            "d1_duplicates": rng.integers(0, 9, size=(300, 1)).astype(np.float32)}


@pytest.mark.parametrize("name", ["constant", "lattice", "constant_column", "huge", "d1_duplicates"])
def test_build_kernel_special_inputs(cuda, name):
    X = special_inputs()[name]
    for psi in (256, 37):
        same(kernel_build(X, 7, psi, 3, 0, cuda), IF.iforest_build_twin(X, 7, psi, 3, 0))


def test_build_kernel_launch_split(cuda):
    X = rows(3)
    a, b = kernel_build(X, 3, 256, 9, 3, cuda), kernel_build(X, 4, 256, 9, 6, cuda)
    whole = kernel_build(X, 7, 256, 9, 3, cuda)
    same(tuple(np.concatenate([p, q]) for p, q in zip(a, b)), whole)
    same(whole, twin(3, 5000, 7, 256, 9, 3))


@lru_cache(maxsize=None)
def scored(D, psi, T=130):
    """A forest of the twin, query rows (training rows and rows outside their range) and the twin's
    path lengths."""
    feat, thr, size = twin(D, 5000, T, psi, 23, 0)
    leaf_c = IF.leaf_c_table(size)
    Q = np.concatenate([rows(D)[:4000], rows(D)[4000:4097] * 3]).astype(np.float32)
    return feat, thr, leaf_c, Q, IF.iforest_path_twin(Q, feat, thr, leaf_c)


@pytest.mark.parametrize("D,psi", [(3, 256), (3, 1000), (33, 256), (64, 1000), (1, 256), (32, 5)])
def test_score_kernel_equals_twin(cuda, D, psi):
    feat, thr, leaf_c, Q, want = scored(D, psi)
    f, t, c = (torch.from_numpy(a).to(cuda) for a in (feat, thr, leaf_c))
    Qd = torch.from_numpy(Q).to(cuda)
    for n in (1, 63, 64, 65, 4097):
        got = C().iforest_score(Qd[:n].contiguous(), f, t, c).cpu().numpy()
        assert np.array_equal(got.view(np.int32), want[:n].view(np.int32)), n
    # a leading-dimension offset (a contiguous view into a larger buffer) is handled
    got = C().iforest_score(Qd[37:1000], f, t, c).cpu().numpy()
    assert np.array_equal(got.view(np.int32), want[37:1000].view(np.int32))
    assert C().iforest_score(Qd[:0], f, t, c).shape == (0,)
    # a non-contiguous view is refused by the binding and handled by the model
    wide = torch.zeros((Q.shape[0], D + 2), device=cuda)
    wide[:, 1:D + 1] = Qd
    with pytest.raises(RuntimeError):
        C().iforest_score(wide[:, 1:D + 1], f, t, c)
    got = IF.path_length(wide[:200, 1:D + 1], f, t, c, psi, True).cpu().numpy()
    assert np.array_equal(got.view(np.int32), want[:200].view(np.int32))


def test_binding_refusals(cuda):
    feat, thr, leaf_c, Q, _ = scored(3, 256)
    f, t, c = (torch.from_numpy(a).to(cuda) for a in (feat, thr, leaf_c))
    X = torch.from_numpy(Q).to(cuda)
    build, score = C().iforest_build, C().iforest_score
    for bad in (lambda: build(X.double(), 4, 16, 0, 0), lambda: build(X[:, 0].contiguous(), 4, 16, 0, 0),
                lambda: build(X.cpu(), 4, 16, 0, 0), lambda: build(X, 4, 1025, 0, 0), lambda: build(X[:10], 4, 16, 0, 0),
                lambda: build(X, 0, 16, 0, 0), lambda: build(X, 4, 0, 0, 0),
                lambda: build(torch.zeros((100, 65), device=cuda), 4, 16, 0, 0),
                lambda: score(X.double(), f, t, c), lambda: score(X, f.long(), t, c), lambda: score(X, f, t.double(), c),
                lambda: score(X, f[:, :100], t[:, :100], c[:, :100]), lambda: score(X, f, t[:5], c),
                lambda: score(X, f, t, c.cpu()), lambda: score(X[:, :2].contiguous(), f, t, c),   # feat holds 2 >= D
                lambda: score(X, f.clamp_max(-2), t, c),
                lambda: score(torch.zeros((10, 65), device=cuda), f, t, c)):
        with pytest.raises((RuntimeError, TypeError)):
            bad()
    f_bad = f.clone()
    f_bad[129, 0] = 3
    with pytest.raises(RuntimeError, match="outside"):
        score(X, f_bad, t, c)
    with pytest.raises(ValueError):
        IsolationForest(engine="philox", use_kernel=True).fit(Q)                          # a CPU tensor
    with pytest.raises(ValueError):
        IsolationForest(engine="philox", use_kernel=True).fit(torch.zeros((300, 65), device=cuda))
    with pytest.raises(ValueError):
        IsolationForest(engine="philox", use_kernel=True, max_samples=1025).fit(torch.from_numpy(rows(3)).to(cuda))


def test_model_outside_the_limits_runs_the_twin(cuda):
    X = np.random.default_rng(5).normal(size=(400, 65)).astype(np.float32)
    a = IsolationForest(n_estimators=5, engine="philox").fit(X)
    b = IsolationForest(n_estimators=5, engine="philox").fit(torch.from_numpy(X).to(cuda))
    assert b.feat.is_cuda and torch.equal(a.feat, b.feat.cpu()) and torch.equal(a.thr, b.thr.cpu())
    assert torch.equal(a.path_length(X), b.path_length(torch.from_numpy(X).to(cuda)).cpu())


def planted(n=2051, d=4, k=20, seed=4):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d))
    X[:k] += rng.choice([-1, 1], size=(k, d)) * 6
    return X.astype(np.float32)


def test_model_cuda_equals_cpu(cuda):
    X = planted()
    cpu = IsolationForest(contamination=0.01, seed=1, engine="philox").fit(X)
    s_cpu = cpu.score_samples(X).numpy()
    assert np.abs(s_cpu - cpu.offset_).min() > 1e-5                   # no training score sits at the offset
    Xd = torch.from_numpy(X).to(cuda)
    gpu = IsolationForest(contamination=0.01, seed=1, engine="philox").fit(Xd)
    assert gpu.feat.is_cuda
    for a, b in ((cpu.feat, gpu.feat), (cpu.thr, gpu.thr), (cpu.size, gpu.size), (cpu.leaf_c, gpu.leaf_c)):
        assert a.dtype == b.dtype and torch.equal(a, b.cpu())
    assert torch.equal(cpu.path_length(X), gpu.path_length(Xd).cpu())
    s_gpu = gpu.score_samples(Xd).cpu().numpy()
    assert np.abs(s_gpu - s_cpu).max() <= 1e-6 * np.abs(s_cpu).min()
    assert abs(gpu.offset_ - cpu.offset_) <= 1e-6 * abs(cpu.offset_)
    p = gpu.predict(Xd).cpu().numpy()
    assert np.array_equal(p, cpu.predict(X).numpy()) and (p[:20] == -1).all()
    forced = IsolationForest(contamination=0.01, seed=1, engine="philox", use_kernel=False).fit(Xd)
    assert forced.feat.is_cuda and torch.equal(forced.feat, gpu.feat)
    assert torch.equal(forced.path_length(Xd), gpu.path_length(Xd))
    # the default engine is the torch forest, as before
    assert IsolationForest(seed=1).fit(Xd).feat.dtype == torch.long


def test_verb_cuda_equals_cpu(cuda, capsys, tmp_path):
    from avenir_amd.cli import main
    props = Path(__file__).parent / "golden" / "iforest" / "iforest.properties"
    X = planted()
    path = tmp_path / "iforest_train.txt"
    path.write_text("".join(f"R{i:04d}," + ",".join(f"{v:.6f}" for v in r) + "\n" for i, r in enumerate(X)))
    Xf = np.loadtxt(path, delimiter=",", usecols=(1, 2, 3, 4)).astype(np.float32)     # the rows as the verb reads them
    m = IsolationForest(contamination=0.01, seed=1, engine="philox").fit(Xf)
    assert np.abs(m.score_samples(Xf).numpy() - m.offset_).min() > 1e-5
    out = {}
    for dev in ("cpu", "cuda"):
        capsys.readouterr()
        assert main(["isolationForest", str(props), f"train.data.file={path}", "train.data.feature.fields=1,2,3,4",
                     "train.contamination=0.01", "train.seed=1", "--device", dev]) == 0
        out[dev] = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    label = {dev: [l.split(",")[2] for l in out[dev][:-1]] for dev in out}
    assert len(label["cpu"]) == len(X) and label["cpu"] == label["cuda"] and out["cpu"][-1] == out["cuda"][-1]
    assert all(v == "-1" for v in label["cuda"][:20])
