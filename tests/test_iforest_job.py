"""The ``isolationForest`` verb (jobs/outlier_jobs.py) on tests/golden/iforest/iforest.properties:
the print format, the planted rows, ``key=value`` overrides and a separate prediction file."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest

from avenir_amd.cli import main
from avenir_amd.models.outlier import IsolationForest

PROPS = Path(__file__).parent / "golden" / "iforest" / "iforest.properties"


def run(capsys, data, device="cpu", **over):
    capsys.readouterr()
    over = {"train.data.file": data, **over}
    assert main(["isolationForest", str(PROPS)] + [f"{k}={v}" for k, v in over.items()] + ["--device", device]) == 0
    return [l for l in capsys.readouterr().out.splitlines() if l.strip()]


@pytest.fixture
def data(tmp_path):
    """An id column and three feature columns; the first 20 rows are planted far from the rest."""
    rng = np.random.default_rng(0)
    X = rng.normal(size=(1000, 3))
    X[:20] += rng.choice([-1, 1], size=(20, 3)) * 6
    p = tmp_path / "iforest_train.txt"
    p.write_text("".join(f"R{i:04d}," + ",".join(f"{v:.6f}" for v in r) + "\n" for i, r in enumerate(X)))
    return p, np.array([[float(f"{v:.6f}") for v in r] for r in X], dtype=np.float32)


def parse(lines, n):
    assert len(lines) == n + 1
    rows = [l.split(",") for l in lines[:-1]]
    assert all(len(r) == 3 for r in rows) and [int(r[0]) for r in rows] == list(range(n))
    score, label = np.array([float(r[1]) for r in rows]), np.array([int(r[2]) for r in rows])
    assert set(label.tolist()) <= {-1, 1} and ((score < 0) & (score >= -1)).all()
    assert lines[-1] == f"num of outliers {(label == -1).sum()}"
    return score, label


def test_isolation_forest_verb(capsys, data):
    path, X = data
    score, label = parse(run(capsys, path), 1000)                     # the file's own settings
    assert (label[:20] == -1).all() and (label == -1).sum() == 20     # contamination 0.02 of 1000 rows
    m = IsolationForest(contamination=0.02, seed=0, engine="philox").fit(X)
    assert np.array_equal(label, m.predict(X).numpy())
    assert np.allclose(score, m.score_samples(X).numpy(), rtol=0, atol=1e-6)


def test_isolation_forest_verb_overrides(capsys, data, tmp_path):
    path, X = data
    over = {"train.num.trees": "20", "train.max.samples": "64", "train.contamination": "auto", "train.seed": "7"}
    score, label = parse(run(capsys, path, **over), 1000)
    m = IsolationForest(n_estimators=20, max_samples=64, seed=7, engine="philox").fit(X)
    assert m.offset_ == -0.5 and tuple(m.feat.shape) == (20, 127)
    assert np.array_equal(label, m.predict(X).numpy()) and (label[:20] == -1).all()
    assert np.allclose(score, m.score_samples(X).numpy(), rtol=0, atol=1e-6)
    assert run(capsys, path, **over) != run(capsys, path, **{**over, "train.seed": "8"})
    # a prediction file: other rows, other columns, scored by the forest of the training file
    Q = np.concatenate([X[5:8], X[500:504]])
    q = tmp_path / "pred.txt"
    q.write_text("".join(",".join(f"{v:.6f}" for v in r) + "\n" for r in Q))
    s2, l2 = parse(run(capsys, path, **over, **{"pred.data.file": q, "pred.data.feature.fields": "0,1,2"}), 7)
    assert np.array_equal(l2, np.concatenate([label[5:8], label[500:504]]))
    assert np.array_equal(s2, np.concatenate([score[5:8], score[500:504]]))
    # scaling never applies
    assert run(capsys, path, **over) == run(capsys, path, **over, **{"common.preprocessing": "scale"})


def test_isolation_forest_verb_rejects(capsys, data):
    path, _ = data
    with pytest.raises(ValueError):
        run(capsys, path, **{"train.contamination": "0.9"})
    with pytest.raises(ValueError):
        run(capsys, path, **{"train.data.feature.fields": "_"})
