"""``isolationForest <properties file> [key=value ...]``: the deterministic isolation forest
(:class:`avenir_amd.models.outlier.IsolationForest` with ``engine="philox"``, the detector behind the
reference's ``DataExplorer.getOutliersWithIsoForest``, P/mlextra/daexp.py:921-941) on a CSV file.

Reads ``train.data.file`` / ``train.data.feature.fields`` (never scaled), ``train.num.trees`` (100),
``train.max.samples`` (``auto``), ``train.contamination`` (``auto``) and ``train.seed`` (0); scores the
rows of ``pred.data.file`` / ``pred.data.feature.fields`` where given (the fields default to the
training fields), else the training rows.  Prints one ``index,score,label`` line per scored row
(label -1 is an outlier) and then ``num of outliers K``.  The device kernels run on a GPU, the numpy
twin on the CPU: the same forest.
"""
from __future__ import annotations

import numpy as np
import torch

from .app_jobs import _Out, _dev, _get, _props, _resolve, _rest
from .cluster_jobs import _data
from .common import job


def _pred_data(conf_path, conf, dev):
    from ..nn.common import load_data_file
    path = _resolve(conf_path, _get(conf, "pred.data.file"))
    if path is None:
        return None
    fields = _get(conf, "pred.data.feature.fields") or _get(conf, "train.data.feature.fields")
    X, _ = load_data_file(path, ",", [int(v) for v in fields.split(",")])
    return torch.from_numpy(X.astype(np.float32)).to(dev)


@job("isolationForest", "isolation forest outlier detection (P/mlextra/daexp.py getOutliersWithIsoForest): "
     "isolationForest <props> [key=value ...]; train.num.trees, train.max.samples, train.contamination, train.seed")
def isolation_forest_verb(args):
    from ..models.outlier import IsolationForest
    rest = _rest(args, 1, "isolationForest <props> [key=value ...]")
    conf, dev = _props(rest[0], rest[1:]), _dev(args)
    conf.pop("common.preprocessing", None)                            # the rows go in unscaled
    ms, cont = str(_get(conf, "train.max.samples", "auto")), str(_get(conf, "train.contamination", "auto"))
    X = _data(rest[0], conf, dev)
    m = IsolationForest(n_estimators=int(_get(conf, "train.num.trees", 100)),
                        max_samples="auto" if ms == "auto" else int(ms),
                        contamination="auto" if cont == "auto" else float(cont),
                        seed=int(_get(conf, "train.seed", 0)), engine="philox").fit(X)
    P = _pred_data(rest[0], conf, dev)
    P = X if P is None else P
    score = m.score_samples(P)
    label = torch.where(score - m.offset_ < 0, -1, 1).cpu().numpy()
    score = score.cpu().numpy()
    out = _Out(args)
    for i in range(len(label)):
        out(f"{i},{score[i]:.6f},{label[i]}")
    out(f"num of outliers {int((label == -1).sum())}")
    out.close()
