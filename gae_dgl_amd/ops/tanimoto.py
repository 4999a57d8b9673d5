"""Exact Tanimoto nearest-neighbour search over bit fingerprints (K34, gae_tanimoto_knn): for every row of ``Q`` the k
rows of ``X`` of the largest |q & x| / |q | x|, without the m x n matrix and without float atomics.  The rows are the
int32 words ``ops.fingerprint_graphs`` returns; ``metrics.knn_predict`` turns the lists into a kNN regressor or
classifier.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import torch

from .._lib import GaeHipError
from ._base import _gpu, _ptr
from ._heads import _search, _search_options

__all__ = ['tanimoto_knn', 'TANIMOTO_MAX_WORDS']

TANIMOTO_MAX_WORDS = 64


def _word_rows(X, who):
    """(X, ldx, n, W): 2-D int32 device bit words as they are when the inner stride is 1, else a contiguous copy"""
    X = _gpu(X, f"{who}: X").detach()
    if X.dtype != torch.int32 or X.dim() != 2:
        raise GaeHipError(f"{who}: int32 bit words [n, W] expected, got {X.dtype} {tuple(X.shape)}")
    n, W = X.shape
    if W > 0 and (X.stride(1) != 1 or (n > 1 and X.stride(0) < W)):
        X = X.contiguous()
    return X, (X.stride(0) if n > 1 else max(W, 1)), n, W


def tanimoto_knn(Q, X=None, k=None, *, exclude_self=None, splits=0):
    """``KNNResult(index int32 [m, k], value fp32 [m, k])``: for every row of ``Q`` [m, W] the ``k`` rows of ``X`` [n, W]
    (int32 bit words on the GPU, read in place through their row stride) of the largest Tanimoto similarity.  With
    a = popcount(q), b = popcount(x), c = popcount(q & x), u = a + b - c the value is the correctly rounded fp32 quotient
    c / u (0.0 when both rows are empty).  Largest first, equal values to the lower row index; rows with fewer than k
    candidates pad with index -1 and value -inf.  ``X=None`` searches ``Q`` against itself and leaves every row out of
    its own list (``exclude_self`` defaults to True then; with a separate ``X`` it must stay off).  ``splits``: column
    splits of the launch, 0 = auto; the result has the same bits for every value.  1 <= W <= 64, 1 <= k <= 64; there is
    no CPU fallback."""
    same, k, flags = _search_options(X, k, exclude_self, splits)
    Q, ldq, m, W = _word_rows(Q, "tanimoto_knn")
    if same:
        X, ldx, n = Q, ldq, m
    else:
        X, ldx, n, wx = _word_rows(X, "tanimoto_knn")
        if wx != W or X.device != Q.device:
            raise GaeHipError(f"tanimoto_knn: X must be [n, {W}] on {Q.device}, got {tuple(X.shape)} on {X.device}")
    return _search("gae_tanimoto_knn", ("tanimoto_knn", m, n, W, k), Q.device, (m, n, W, k, int(splits)),
                   (_ptr(Q), ldq, m, _ptr(X), ldx, n, W, k, flags, int(splits)))
