"""fp64 restatement of gae_knn's contract (include/gae_hip_experimental.h, K24), written from the header: brute force
over every (query, database row) pair in numpy.

Candidates of query i: the database rows j whose key is finite -- here: x_j and q_i hold neither NaN nor inf -- minus
j = i under ``exclude_same``.  "l2": value = sum_f (q_if - x_jf)^2, rows sorted by (value ascending, j ascending);
"dot": value = q_i . x_j, rows sorted by (value descending, j ascending).  Fewer than k candidates pad with index -1
and value +inf (l2) / -inf (dot)."""
import numpy as np

CHUNK = 512          # queries per block of the distance matrix


def _finite_rows(A):
    return np.isfinite(A).all(axis=1) if A.shape[0] else np.zeros(0, bool)


def scores(Q, X, metric, rows=None):
    """fp64 [len(rows), n]: the value of every pair, +inf (l2) / -inf (dot) where the pair is no candidate for lack of a
    finite key.  ``rows``: the queries asked for (default all)."""
    Q, X = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    rows = np.arange(Q.shape[0]) if rows is None else np.asarray(rows)
    okx, okq = _finite_rows(X), _finite_rows(Q)
    Xc, Qc = np.where(okx[:, None], X, 0.0), np.where(okq[:, None], Q, 0.0)[rows]
    bad = np.inf if metric == "l2" else -np.inf
    if metric == "l2":
        V = (Qc * Qc).sum(1)[:, None] - 2.0 * (Qc @ Xc.T) + (Xc * Xc).sum(1)[None, :]
        V = np.maximum(V, 0.0)
    else:
        V = Qc @ Xc.T
    V[:, ~okx] = bad
    V[~okq[rows], :] = bad
    return V


def pair_values(Q, X, index, metric, rows=None):
    """fp64, the shape of ``index``: the value of (query, index) taken directly; padding gets +inf / -inf"""
    Q, X = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    rows = np.arange(Q.shape[0]) if rows is None else np.asarray(rows)
    idx = np.asarray(index, np.int64)
    out = np.full(idx.shape, np.inf if metric == "l2" else -np.inf)
    if X.shape[0] == 0:
        return out
    q = Q[rows][:, None, :]
    x = X[np.maximum(idx, 0)]
    with np.errstate(invalid="ignore", over="ignore"):
        v = ((q - x) ** 2).sum(-1) if metric == "l2" else (q * x).sum(-1)
    return np.where(idx >= 0, v, out)


def knn(Q, X, k, metric="l2", exclude_same=False):
    """(index int32 [m, k], value fp64 [m, k]): the exact k nearest by (value, j), with the padding rule"""
    Q, X = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    m, n = Q.shape[0], X.shape[0]
    pad = np.inf if metric == "l2" else -np.inf
    index = np.full((m, k), -1, np.int32)
    for r0 in range(0, m, CHUNK):
        rows = np.arange(r0, min(r0 + CHUNK, m))
        V = scores(Q, X, metric, rows)
        if exclude_same:
            inside = rows < n
            V[np.nonzero(inside)[0], rows[inside]] = pad
        key = V if metric == "l2" else -V
        order = np.argsort(key, axis=1, kind="stable")[:, :k]          # stable: equal values keep ascending j
        taken = np.take_along_axis(V, order, 1)
        kk = order.shape[1]
        index[rows, :kk] = np.where(np.isfinite(taken), order, -1)
    return index, pair_values(Q, X, index, metric)


def tolerance(Q, X):
    """T_i = 2 (d + 2) 2^-24 (|q_i|^2 + max_j |x_j|^2): the fmaf-chain bound on the expanded fp32 key q . x - |x|^2 / 2,
    expressed on the distance |q - x|^2 = |q|^2 - 2 key.  The chains of q . x and |x|^2 take d roundings each and the
    halving and the subtraction one more, every one within 2^-24 of a partial sum that |q| |x| <= (|q|^2 + |x|^2) / 2
    bounds; doubled for the higher-order terms"""
    Q, X = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    d = Q.shape[1]
    xmax = float((X * X).sum(1).max()) if X.shape[0] else 0.0
    return 2.0 * (d + 2) * 2.0 ** -24 * ((Q * Q).sum(1) + xmax)


def check_tolerant(Q, X, index, value, exclude_same=False, rows=None):
    """The l2 result ``index`` / ``value`` [len(rows), k] against fp64, row by row, no row exempt.  With D the fp64
    distance and D_i(k) its k-th smallest over the candidates: every returned j has D_ij <= D_i(k) + 2 T_i, every j with
    D_ij < D_i(k) - 2 T_i is returned, no j repeats, padding only where there are fewer than k candidates, and the
    reported values ascend.  Returns a list of messages, empty when all holds."""
    Q, X = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    index, value = np.asarray(index), np.asarray(value)
    rows = np.arange(Q.shape[0]) if rows is None else np.asarray(rows)
    k, n = index.shape[1], X.shape[0]
    T = tolerance(Q, X)[rows]
    bad = []
    for c0 in range(0, len(rows), CHUNK):
        sl = slice(c0, min(c0 + CHUNK, len(rows)))
        rr = rows[sl]
        D = scores(Q, X, "l2", rr)
        if exclude_same:
            D[np.arange(len(rr)), rr] = np.inf
        idx, val, t = index[sl].astype(np.int64), value[sl], T[sl]
        n_cand = np.isfinite(D).sum(1)
        want = np.minimum(n_cand, k)
        got = (idx >= 0).sum(1)
        if (got != want).any() or ((idx >= 0) != (np.arange(k)[None, :] < want[:, None])).any():
            bad.append(f"rows {rr[got != want][:5]}: valid entries {got[got != want][:5]}, candidates allow {want[got != want][:5]}")
            continue
        if (want == k).all():
            Dk = np.partition(D, k - 1, axis=1)[:, k - 1]               # the k-th smallest
        else:
            Dk = np.sort(D, axis=1)[np.arange(len(rr)), np.maximum(want, 1) - 1]      # ... or the last candidate
        Dk = np.where(want > 0, Dk, np.inf)
        Dret = np.where(idx >= 0, np.take_along_axis(D, np.maximum(idx, 0), 1), -np.inf)
        over = Dret > (Dk + 2 * t)[:, None]
        if over.any():
            r = np.nonzero(over.any(1))[0][0]
            bad.append(f"row {rr[r]}: returned D {Dret[r].max():.9g} > D(k) {Dk[r]:.9g} + 2 T {2 * t[r]:.3g}")
        must = D < (Dk - 2 * t)[:, None]
        have = np.zeros_like(must)
        np.put_along_axis(have, np.maximum(idx, 0), idx >= 0, 1)
        if (must & ~have).any():
            r = np.nonzero((must & ~have).any(1))[0][0]
            bad.append(f"row {rr[r]}: {np.nonzero(must[r] & ~have[r])[0][:5]} lie clearly inside D(k) and are missing")
        srt = np.sort(np.where(idx >= 0, idx, -1 - np.arange(k)[None, :]), axis=1)
        if (srt[:, 1:] == srt[:, :-1]).any():
            bad.append(f"rows {rr[(srt[:, 1:] == srt[:, :-1]).any(1)][:5]}: a repeated index")
        if (np.diff(val.astype(np.float64), axis=1) < 0).any():
            bad.append(f"rows {rr[(np.diff(val.astype(np.float64), axis=1) < 0).any(1)][:5]}: values not ascending")
        if (idx >= n).any() or (exclude_same and (idx == rr[:, None]).any()):
            bad.append("an index out of range or a row in its own list")
    return bad


def expanded_fp32(Q, X, index, rows=None):
    """what an implementation that REPORTS the expanded form |q|^2 - 2 q . x + |x|^2 in fp32 would return for the
    pairs of ``index``: the cancellation the contract keeps out of the output"""
    Q, X = np.asarray(Q, np.float32), np.asarray(X, np.float32)
    rows = np.arange(Q.shape[0]) if rows is None else np.asarray(rows)
    idx = np.maximum(np.asarray(index, np.int64), 0)
    q, x = Q[rows][:, None, :], X[idx]
    qn = (q * q).sum(-1, dtype=np.float32)
    xn = (x * x).sum(-1, dtype=np.float32)
    p = (q * x).sum(-1, dtype=np.float32)
    return (qn - np.float32(2) * p + xn).astype(np.float32)
