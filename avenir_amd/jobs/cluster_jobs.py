"""``cluster <properties file> [key=value ...]``: the density-clustering half of the reference's
P/unsupv/cluster.py driver, in the script's print formats.

* ``common.mode=train``, ``train.algo=dbscan``: :class:`avenir_amd.models.dbscan.DBSCAN` (the device
  kernels on a GPU, the numpy twin on the CPU: the same bits).  The reference tests ``cl > 0`` where
  it means a cluster, which files cluster 0 under noise; here a label >= 0 is a cluster.
* ``common.mode=explore``, ``expl.algo=kdist``: the ascending sorted distances to neighbour k of
  every point (the point itself excluded), for k below ``expl.kdist.neighbor.index``.
* ``common.mode=explore``, ``expl.algo=hopkins``: ``cluster.hopkins`` once per
  ``expl.hopkins.num.iters`` with seeds 0, 1, ..., and the mean.

``train.algo=kmeans`` is the ``kmeansCluster`` verb and ``train.algo=agglomerative`` the
``agglomerativeCluster`` verb below; ``common.mode=predict`` is not supported.

``agglomerativeCluster <properties file> [key=value ...]`` reads the same file: the data keys above,
the first entry of ``train.num.clusters``, ``train.affinity`` (``default`` means euclidean),
``train.linkage`` and ``train.output.cluster.members``, and runs
:class:`avenir_amd.models.agglo.AgglomerativeClustering` whatever ``common.mode`` and ``train.algo`` say.
"""
from __future__ import annotations

import numpy as np
import torch

from .app_jobs import _Out, _bool, _dev, _get, _props, _resolve, _rest
from .common import job


def _data(conf_path, conf, dev) -> torch.Tensor:
    """Columns ``train.data.feature.fields`` of ``train.data.file`` as fp32; ``common.preprocessing=
    scale`` standardises every column first (column mean, population standard deviation, fp64)."""
    from ..nn.common import load_data_file
    path = _resolve(conf_path, _get(conf, "train.data.file"))
    fields = _get(conf, "train.data.feature.fields")
    if path is None or fields is None:
        raise ValueError("train.data.file and train.data.feature.fields are required")
    X, _ = load_data_file(path, ",", [int(v) for v in fields.split(",")])
    if _get(conf, "common.preprocessing") == "scale":
        sd = X.std(0)
        X = (X - X.mean(0)) / np.where(sd > 0, sd, 1.0)
    return torch.from_numpy(X.astype(np.float32)).to(dev)


def _train_dbscan(conf, X, out):
    from ..models.dbscan import DBSCAN
    eps, ms = float(_get(conf, "train.eps", -1)), int(_get(conf, "train.min.samples", -1))
    metric = _get(conf, "train.metric", "default")
    out("starting dbscan clustering...")
    m = DBSCAN(eps=0.5 if eps < 0 else eps, min_samples=5 if ms < 0 else ms,
               metric="euclidean" if metric == "default" else metric).fit(X)
    core = m.core_sample_indices_.cpu().tolist()
    if _bool(conf, "train.output.core.points"):
        out("core points data index")
        out(str(core))
    out(f"num of core points {len(core)}")
    out("all points clutser index")
    labels = m.labels_.cpu().numpy()
    if _bool(conf, "train.output.cluster.members"):
        noise = np.flatnonzero(labels < 0).tolist()
        if noise:
            out(f"noise points size {len(noise)}")
            out(str(noise))
        for c in range(m.n_clusters_):
            members = np.flatnonzero(labels == c).tolist()
            out(f"cluster index {c}  size {len(members)}")
            out(str(members))
    out(f"num of clusters {m.n_clusters_}")


def _train_agglomerative(conf, X, out):
    from ..models.agglo import AgglomerativeClustering
    k = int(str(_get(conf, "train.num.clusters", "2")).split(",")[0])
    affinity, link = _get(conf, "train.affinity", "default"), _get(conf, "train.linkage", "default")
    out("starting agglomerative clustering...")
    m = AgglomerativeClustering(n_clusters=k, metric="euclidean" if affinity == "default" else affinity,
                                linkage="ward" if link == "default" else link).fit(X)
    labels = m.labels_.cpu().numpy()
    out(str(labels.tolist()))
    if _bool(conf, "train.output.cluster.members"):
        for c in range(m.n_clusters_):
            members = np.flatnonzero(labels == c).tolist()
            out(f"cluster index {c}  size {len(members)}")
            out(str(members))
    out(f"num of clusters {m.n_clusters_}")


def _expl_kdist(conf, X, out):
    from ..ops import distance as dist
    k = int(_get(conf, "expl.kdist.neighbor.index"))
    if not 1 <= k < X.shape[0]:
        raise ValueError("expl.kdist.neighbor.index must lie in 1 .. n - 1")
    out("calculating distance to nearest kth neighbor ...")
    d, _ = dist.knn(X, X, k, exclude_self=True)
    d = d.sort(0).values.cpu().numpy()
    out("after sorting")
    diff = _bool(conf, "expl.kdist.output.dist.first.order.diff")
    for j in range(k):
        out(f"sorted distance to nearest neighbor at position {j} ")
        out(" ".join(f"{v:.6f}" for v in d[:, j]))
        if diff:
            out("1st order diff of sorted distance to kth neighbor")
            out(" ".join(f"{v:.6f}" for v in np.diff(d[:, j])))


def _expl_hopkins(conf, X, out):
    from ..models import cluster
    sample, iters = int(_get(conf, "expl.hopkins.sample.size", 100)), int(_get(conf, "expl.hopkins.num.iters", 1))
    out("calculating hopkins stats to detect if the data set has clusters...")
    stats = [cluster.hopkins(X, sample, seed) for seed in range(iters)]
    for h in stats:
        out(f"hopkins stats {h:.3f}")
    out(f"average hopkins stat {float(np.mean(stats)):.3f}")


@job("cluster", "density clustering driver (P/unsupv/cluster.py): cluster <props> [key=value ...]; train.algo=dbscan, "
     "expl.algo=kdist | hopkins")
def cluster_verb(args):
    rest = _rest(args, 1, "cluster <props> [key=value ...]")
    conf, dev = _props(rest[0], rest[1:]), _dev(args)
    mode = _get(conf, "common.mode")
    if mode == "train":
        algo = _get(conf, "train.algo")
        if algo == "kmeans":
            raise ValueError("train.algo=kmeans is the kmeansCluster verb")
        if algo != "dbscan":
            raise ValueError(f"unsupported cluster algorithm {algo} (train.algo=dbscan; k-means is the kmeansCluster verb)")
        out = _Out(args)
        out("running in training mode...")
        _train_dbscan(conf, _data(rest[0], conf, dev), out)
    elif mode == "explore":
        algo = _get(conf, "expl.algo")
        if algo not in ("kdist", "hopkins"):
            raise ValueError("invalid cluster exploration algorithm")
        out = _Out(args)
        out("running in explore mode...")
        (_expl_kdist if algo == "kdist" else _expl_hopkins)(conf, _data(rest[0], conf, dev), out)
    else:
        raise ValueError(f"unsupported mode {mode} (common.mode=train | explore)")
    out.close()


@job("agglomerativeCluster", "agglomerative clustering (P/unsupv/cluster.py, train.algo=agglomerative): "
     "agglomerativeCluster <props> [key=value ...]; train.num.clusters, train.affinity, train.linkage")
def agglomerative_cluster_verb(args):
    rest = _rest(args, 1, "agglomerativeCluster <props> [key=value ...]")
    conf, dev = _props(rest[0], rest[1:]), _dev(args)
    out = _Out(args)
    _train_agglomerative(conf, _data(rest[0], conf, dev), out)
    out.close()
