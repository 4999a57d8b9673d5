"""Exact nearest-neighbour search over embeddings (K24, gae_knn): for every row of ``Q`` the k nearest rows of ``X`` under
squared Euclidean distance, inner product or cosine similarity, without the m x n matrix and without float atomics.
``GAE.nearest_nodes``, ``GAE.nearest_graphs``; ``metrics.knn_predict`` turns the neighbours into a kNN regressor or
classifier.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import collections

import torch

from .. import _lib
from .._lib import GaeHipError
from ._base import _on_device, _ptr, _stream, _timed, _ws_bytes
from ._heads import _rows

__all__ = ['KNNResult', 'knn', 'KNN_MAX_K', 'KNN_MAX_D', 'KNN_MAX_SPLITS']

KNNResult = collections.namedtuple("KNNResult", ["index", "value"])
KNNResult.__doc__ = """index int32 [m, k] (rows of the database, -1 = padding), value fp32 [m, k]: the squared distance
("l2", ascending), the inner product ("dot") or the cosine ("cosine"), both descending; padding holds +inf / -inf"""

KNN_MAX_K, KNN_MAX_D, KNN_MAX_SPLITS = 64, 256, 16
_METRICS = {"l2": _lib.KNN_L2, "dot": _lib.KNN_DOT, "cosine": _lib.KNN_DOT}


def _unit_rows(X, who):
    norm = torch.linalg.vector_norm(X, dim=1, keepdim=True)
    if X.shape[0] and not bool((norm > 0).all()):
        raise GaeHipError(f"{who}: metric 'cosine' with a zero row")
    return X / norm


def knn(Q, X=None, k=None, *, metric="l2", exclude_self=None, splits=0):
    """``KNNResult(index, value)``: for every row of ``Q`` [m, d] the ``k`` nearest rows of ``X`` [n, d] (fp32, on the
    GPU; read in place when the inner stride is 1).  ``metric``: "l2" (squared Euclidean distance, smallest first; the
    reported distance is taken directly, sum_f (q_f - x_f)^2), "dot" (inner product, largest first) or "cosine" (the
    rows are divided by their norms here and searched by "dot"; a zero row is an error).  Equal values go to the lower
    row index; rows with fewer than k candidates pad with index -1.  A database row that holds NaN or inf is never
    returned.  ``X=None`` searches ``Q`` against itself and leaves every row out of its own list (``exclude_self``
    defaults to True then; with a separate ``X`` it must stay off).  ``splits``: column splits of the launch, 0 = auto;
    the result has the same bits for every value.  1 <= d <= 256, 1 <= k <= 64; there is no CPU fallback."""
    if metric not in _METRICS:
        raise ValueError(f"metric: 'l2', 'dot' or 'cosine', not {metric!r}")
    if k is None or isinstance(k, bool) or int(k) != k:
        raise ValueError(f"k: an integer in 1..{KNN_MAX_K}, not {k!r}")
    if isinstance(splits, bool) or int(splits) != splits or not 0 <= splits <= KNN_MAX_SPLITS:
        raise ValueError(f"splits: 0 (auto) or 1..{KNN_MAX_SPLITS}, not {splits!r}")
    same = X is None
    if exclude_self is None:
        exclude_self = same
    if exclude_self and not same:
        raise ValueError("exclude_self needs X=None: rows of a separate X share no index with the queries")
    k = int(k)
    with torch.no_grad():
        Q, ldq, m, d = _rows(Q, "knn")
        if metric == "cosine":
            Q, ldq = _unit_rows(Q, "knn"), max(d, 1)
        if same:
            X, ldx, n = Q, ldq, m
        else:
            X, ldx, n, dx = _rows(X, "knn")
            if dx != d or X.device != Q.device:
                raise GaeHipError(f"knn: X must be [n, {d}] on {Q.device}, got {tuple(X.shape)} on {X.device}")
            if metric == "cosine":
                X, ldx = _unit_rows(X, "knn"), max(d, 1)
        dev = Q.device
        kk = max(k, 1)
        index = torch.empty(m, kk, dtype=torch.int32, device=dev)
        value = torch.empty(m, kk, dtype=torch.float32, device=dev)
        flags = _lib.KNN_EXCLUDE_SAME_INDEX if exclude_self else 0
        with _on_device(dev):
            nbytes = _ws_bytes("gae_knn_workspace_bytes", m, n, d, k, int(splits))
            ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)

            def launch():
                _lib.call("gae_knn", _ptr(Q), ldq, m, _ptr(X), ldx, n, d, k, _METRICS[metric], flags, int(splits),
                          _ptr(index), _ptr(value), kk, _ptr(ws), ws.numel(), _stream())
            _timed(("knn", m, n, d, k), launch)
    return KNNResult(index, value)
