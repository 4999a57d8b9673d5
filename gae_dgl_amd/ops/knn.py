"""Exact nearest-neighbour search over embeddings (K24, gae_knn): for every row of ``Q`` the k nearest rows of ``X`` under
squared Euclidean distance, inner product or cosine similarity, without the m x n matrix and without float atomics.
``GAE.nearest_nodes``, ``GAE.nearest_graphs``; ``metrics.knn_predict`` turns the neighbours into a kNN regressor or
classifier.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import torch

from .. import _lib
from .._lib import GaeHipError
from ._base import _ptr
from ._heads import KNN_MAX_K, KNN_MAX_SPLITS, KNNResult, _rows, _search, _search_options

__all__ = ['KNNResult', 'knn', 'KNN_MAX_K', 'KNN_MAX_D', 'KNN_MAX_SPLITS']

KNN_MAX_D = 256
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
    same, k, flags = _search_options(X, k, exclude_self, splits)
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
        return _search("gae_knn", ("knn", m, n, d, k), Q.device, (m, n, d, k, int(splits)),
                       (_ptr(Q), ldq, m, _ptr(X), ldx, n, d, k, _METRICS[metric], flags, int(splits)))
