"""Dense numpy fp64 reference of gae_decoder_threshold_count / _fill (K22) for the tests: the CSR of include/
gae_hip_experimental.h read off full rows of Z Z^T.  O(n^2) work -- test sizes only; nothing here is on a product path.

    indptr, index, score = threshold_ref(Z, threshold, windows=None, csr=None, exclude_self=True)

``Z``: [n, d] array (taken to fp64); ``windows``: int [n, 2] member window [w0, w1) of every node, or None (all n);
``csr``: host (indptr, indices) whose row i is left out of i's candidates (any order, repeats allowed), or None.
Row i lists, columns ascending, the candidates c with s_ic >= threshold; NaN and -inf scores are never listed."""
import numpy as np

from rank_ref import candidate_row


def threshold_ref(Z, threshold, windows=None, csr=None, exclude_self=True, scores=None):
    """(indptr int64 [n + 1], index int64 [nnz], score fp64 [nnz]).  ``scores``: an [n, n] matrix to read the logits
    from instead of Z Z^T (recorded reference logits, or the fp32 chain of the kernels)."""
    Z = np.asarray(Z, dtype=np.float64)
    n = Z.shape[0] if scores is None else scores.shape[0]
    indptr = np.zeros(n + 1, dtype=np.int64)
    cols, vals = [], []
    for i in range(n):
        with np.errstate(invalid="ignore", over="ignore"):
            s = Z @ Z[i] if scores is None else np.asarray(scores[i], dtype=np.float64)
        ok = candidate_row(n, i, windows, csr, exclude_self)
        ok &= ~np.isnan(s) & (s != -np.inf)
        with np.errstate(invalid="ignore"):
            ok &= s >= threshold
        c = np.flatnonzero(ok)
        cols.append(c)
        vals.append(s[c])
        indptr[i + 1] = indptr[i] + c.size
    index = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    score = np.concatenate(vals) if vals else np.zeros(0, np.float64)
    return indptr, index.astype(np.int64), score.astype(np.float64)


def dense_mask(indptr, index, n):
    """bool [n, n] of a CSR"""
    A = np.zeros((n, n), dtype=bool)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    A[rows, index] = True
    return A
