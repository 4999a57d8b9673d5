"""Dense numpy fp64 reference of gae_decoder_rank (K18) for the tests: the counts of include/gae_hip_experimental.h read
off a full row of Z Z^T per query.  O(m n) memory in chunks -- test sizes only; nothing here is on a product path.

    score, greater, equal, candidates = rank_ref(Z, src, dst, windows=None, csr=None, exclude_self=True)

``Z``: [n, d] array (taken to fp64); ``windows``: int [n, 2] member window [w0, w1) of every node, or None (all n);
``csr``: host (indptr, indices) whose row i is left out of i's candidates (any order, repeats count once), or None.
A query with an index outside [0, n) gives NaN and -1s."""
import numpy as np


def candidate_row(n, i, windows=None, csr=None, exclude_self=True):
    """bool [n]: the columns of node i's window that are neither i (exclude_self) nor in CSR row i"""
    ok = np.ones(n, dtype=bool)
    if windows is not None:
        c = np.arange(n)
        ok &= (c >= windows[i, 0]) & (c < windows[i, 1])
    if exclude_self:
        ok[i] = False
    if csr is not None:
        indptr, indices = csr
        row = np.asarray(indices[indptr[i]:indptr[i + 1]], dtype=np.int64)
        ok[row[(row >= 0) & (row < n)]] = False
    return ok


def rank_ref(Z, src, dst, windows=None, csr=None, exclude_self=True, scores=None):
    """(score fp64 [m], greater int64 [m], equal int64 [m], candidates int64 [m]).  ``scores``: an [n, n] matrix to
    read the logits from instead of Z Z^T (recorded reference logits)."""
    Z = np.asarray(Z, dtype=np.float64)
    n = Z.shape[0] if scores is None else scores.shape[0]
    src = np.asarray(src, dtype=np.int64).reshape(-1)
    dst = np.asarray(dst, dtype=np.int64).reshape(-1)
    m = src.size
    score = np.full(m, np.nan)
    greater = np.full(m, -1, dtype=np.int64)
    equal = np.full(m, -1, dtype=np.int64)
    cand = np.full(m, -1, dtype=np.int64)
    for q in range(m):
        i, j = int(src[q]), int(dst[q])
        if not (0 <= i < n and 0 <= j < n):
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            s = Z @ Z[i] if scores is None else np.asarray(scores[i], dtype=np.float64)
        ok = candidate_row(n, i, windows, csr, exclude_self)
        ok &= ~np.isnan(s) & (s != -np.inf)
        ok[j] = False                                  # the target is never counted against itself
        t = s[j]
        score[q] = t
        cand[q] = int(ok.sum())
        if np.isnan(t):
            greater[q], equal[q] = cand[q], 0
        else:
            greater[q] = int((s[ok] > t).sum())
            equal[q] = int((s[ok] == t).sum())
    return score, greater, equal, cand
