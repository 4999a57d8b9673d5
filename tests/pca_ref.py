"""numpy restatement of K31 (gae_pca_solve / gae_pca_transform, ops.pca), written from the K31 comment of
include/gae_hip_experimental.h: the centring, the round-robin ordering, every rotation as a sequence of single fp64
operations, the order inside a round (column rotation, then row rotation, the mirror a copy), the stopping rule, the
ordering and the sign rule; the projection as one fp32 fma chain per score (tests/mlp_ref.py's chain).  The device must
return the same bits.  ``direct`` is the independent answer (fp64 covariance and LAPACK).  Shared by
tests/test_pca_cpu.py and tests/test_gpu_pca.py."""
import collections

import numpy as np

from mlp_ref import chain

f32, f64 = np.float32, np.float64
MAX_SWEEPS = 30
TOL = 2.0 ** -53

Solved = collections.namedtuple("Solved", ["mean", "values", "components", "info", "n_sweeps", "n_rotations", "off_norm",
                                           "total_variance", "all_values", "all_components", "cov"])


# (name, n, d, k, kind): the smallest shapes at which the kernels can go wrong -- odd d (an index sits out), the 16-wide
# tile edges, the LDS limit d = 128, V in LDS (d <= 96) and in the workspace (d = 97 on), n_used on both sides of K25's
# 256-row chunk
CASES = [
    ("d1", 2, 1, 1, "plain"), ("d2", 5, 2, 2, "plain"), ("d3", 5, 3, 1, "plain"), ("d3n2", 2, 3, 3, "plain"),
    ("d2n1000", 1000, 2, 1, "plain"), ("d16", 255, 16, 2, "plain"), ("d16k1", 1000, 16, 1, "plain"),
    ("d17", 257, 17, 17, "plain"), ("d48", 1000, 48, 48, "plain"), ("d127", 257, 127, 2, "plain"),
    ("d96", 257, 96, 2, "plain"), ("d97", 255, 97, 97, "plain"), ("d127full", 1000, 127, 127, "plain"), ("d128", 1000, 128, 128, "plain"), ("d128k1", 255, 128, 1, "plain"),
    ("rank3", 3, 16, 16, "plain"), ("dupcol", 255, 17, 17, "dup"), ("constcol", 257, 16, 16, "const"),
    ("bigmean", 257, 48, 2, "bigmean"), ("subset", 255, 17, 2, "subset"),
]


def make(case):
    """(X fp32 [n_total, d], rows int64 ids or None, k) of a case: correlated columns of unequal spread, from a seed of
    the case's own"""
    name, n, d, k, kind = case
    rng = np.random.default_rng(sum(name.encode()) * 1000 + n + d)
    X = rng.standard_normal((n, d)) * rng.uniform(0.1, 3.0, d)
    if d >= 3:
        X = X @ (np.eye(d) + 0.3 * rng.standard_normal((d, d)))
    rows = None
    if kind == "dup":
        X[:, 5] = X[:, 11]
    elif kind == "const":
        X[:, 7] = 2.5
    elif kind == "bigmean":
        X = rng.standard_normal((n, d)) + 1e4 + 10.0 * rng.standard_normal(d)
    elif kind == "subset":
        total = 400
        rows = np.sort(rng.permutation(total)[:n])
        full = np.full((total, d), np.nan)
        full[::3] = 1e30
        full[rows] = X
        X = full
    return X.astype(f32), rows, k


def upper_at(i, j, W):
    return i * W - i * (i - 1) // 2 + (j - i)


def unpack(stats, W):
    """the symmetric [W, W] matrix of one fold's packed upper triangle"""
    M = np.zeros((W, W), f64)
    iu = np.triu_indices(W)
    M[iu] = np.asarray(stats, f64).reshape(-1)[:W * (W + 1) // 2]
    return np.triu(M) + np.triu(M, 1).T


def moments(X, pivot=None, t=1):
    """K25's packed moments of the rows of X with Y = column 0 (t = 1), by plain fp64 numpy: the device's own stats differ
    from these in the order of the sums only (the CPU tests start here, the GPU tests from the device's stats)"""
    X = np.asarray(X, f32)
    n, d = X.shape
    p = np.zeros(d + t, f32) if pivot is None else np.asarray(pivot, f32)
    V = np.concatenate([np.ones((n, 1)), X.astype(f64) - p[:d].astype(f64),
                        X[:, :1].astype(f64).repeat(t, 1) - p[d:d + t].astype(f64)], 1)
    M = V.T @ V
    return M[np.triu_indices(1 + d + t)]


def centre(stats, d, t, pivot):
    """(c, mean, C): C_ij = C_ji = (S_ij - s_j mu_i) / (c - 1) for i <= j, product rounded before the difference"""
    W = 1 + d + t
    S = unpack(stats, W)
    c = S[0, 0]
    s = S[0, 1:1 + d].copy()
    with np.errstate(all="ignore"):
        mu = s / c
        U = (S[1:1 + d, 1:1 + d] - s[None, :] * mu[:, None]) / (c - 1.0)    # entry (i, j): s_j mu_i -- used for i <= j
    C = np.triu(U) + np.triu(U, 1).T
    p = np.zeros(d, f64) if pivot is None else np.asarray(pivot, f32)[:d].astype(f64)
    return c, p + mu, C


def pairs(dp, r):
    """the round's pairs (p, q), p < q, pair 0 first; index dp - 1 is the fixed player"""
    out = [(r, dp - 1)]
    for k in range(1, dp // 2):
        x, y = (r + k) % (dp - 1), (r - k) % (dp - 1)
        out.append((min(x, y), max(x, y)))
    return out


def jacobi(C):
    """(A, Vt, info, n_sweeps, n_rotations): Vt's row i is column i of V.  An odd d is padded with a zero row and column:
    the pair of the padding index is never rotated (a_pq == 0), which is the index sitting out"""
    d = C.shape[0]
    dp = d + (d & 1)
    m = dp // 2
    A = np.zeros((dp, dp), f64)
    A[:d, :d] = C
    Vt = np.eye(dp, dtype=f64)
    rounds = [np.array(pairs(dp, r)) for r in range(dp - 1)]
    info, sweeps, total = 1, 0, 0
    with np.errstate(all="ignore"):
        for _ in range(MAX_SWEEPS):
            before = total
            for pq in rounds:
                p, q = pq[:, 0], pq[:, 1]
                app, aqq, apq = A[p, p], A[q, q], A[p, q]
                rot = (apq != 0.0) & (np.abs(apq) > TOL * np.sqrt(np.abs(app) * np.abs(aqq)))
                if not rot.any():
                    continue
                safe = np.where(rot, apq, 1.0)
                tau = (aqq - app) / (2.0 * safe)
                t = np.where(tau >= 0.0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
                t, c, s = np.where(rot, t, 0.0), np.where(rot, c, 1.0), np.where(rot, s, 0.0)
                total += int(rot.sum())
                # column rotation on every row, then row rotation on every column
                B = A.copy()
                B[:, p] = c * A[:, p] - s * A[:, q]
                B[:, q] = s * A[:, p] + c * A[:, q]
                D = B.copy()
                D[p, :] = c[:, None] * B[p, :] - s[:, None] * B[q, :]
                D[q, :] = s[:, None] * B[p, :] + c[:, None] * B[q, :]
                # blocks of pairs k < l are computed, their transposes copied
                pid = np.empty(dp, np.int64)
                pid[p] = np.arange(m)
                pid[q] = np.arange(m)
                upper = pid[:, None] < pid[None, :]
                new = np.where(upper, D, D.T)
                # a pair's own block
                own = pid[:, None] == pid[None, :]
                new[own] = A[own]
                delta = t * apq
                pr, qr = p[rot], q[rot]
                new[pr, pr] = app[rot] - delta[rot]
                new[qr, qr] = aqq[rot] + delta[rot]
                new[pr, qr] = 0.0
                new[qr, pr] = 0.0
                A = new
                vp, vq = Vt[p, :].copy(), Vt[q, :].copy()
                Vt[p, :] = c[:, None] * vp - s[:, None] * vq
                Vt[q, :] = s[:, None] * vp + c[:, None] * vq
            sweeps += 1
            if total == before:
                info = 0
                break
    return A[:d, :d], Vt[:d, :d], info, sweeps, total


def finish(A, Vt):
    """(all values descending -- equal values to the lower index --, all components with the sign rule, off_norm)"""
    d = A.shape[0]
    lam = np.diag(A).copy()
    order = sorted(range(d), key=lambda i: (np.isnan(lam[i]), -lam[i], i))   # (a NaN sorts last)
    comps = Vt[order, :].copy()
    for r in range(d):
        at = int(np.argmax(np.abs(comps[r])))                               # the first of equal magnitudes
        if comps[r, at] < 0.0:
            comps[r] = -comps[r]
    rowsum = np.zeros(d, f64)
    for j in range(d):                                                      # j ascending, the diagonal left out
        sq = A[:, j] * A[:, j]
        rowsum = np.where(np.arange(d) == j, rowsum, rowsum + sq)
    off = f64(0.0)
    for i in range(d):
        off = off + rowsum[i]
    return lam[order], comps, np.sqrt(off)


def solve(stats, d, t, pivot, k):
    """what gae_pca_solve writes for one fold's packed moments"""
    c, mean, C = centre(stats, d, t, pivot)
    nan = np.full
    if not c >= 2.0:
        return Solved(nan(d, np.nan), nan(k, np.nan), nan((k, d), np.nan), -1, 0, 0, np.nan, np.nan, None, None, C)
    A, Vt, info, sweeps, rotations = jacobi(C)
    values, comps, off = finish(A, Vt)
    total = f64(0.0)
    for v in values:
        total = total + v
    if info != 0:
        return Solved(nan(d, np.nan), nan(k, np.nan), nan((k, d), np.nan), info, sweeps, rotations, np.nan, np.nan,
                      values, comps, C)
    return Solved(mean, values[:k].copy(), comps[:k].copy(), info, sweeps, rotations, off, total, values, comps, C)


def transform(X, mean, components, values=None, whiten=False, rows=None):
    """fp32 [n_rows, k]: gae_pca_transform's scores -- m and v rounded to fp32 once, x - m one fp32 operation, one fma
    chain over j ascending; a listed row that holds a non-finite value is a NaN row"""
    X = np.asarray(X, f32)
    if rows is not None:
        X = X[np.asarray(rows, np.int64)]
    m32, v32 = np.asarray(mean, f64).astype(f32), np.asarray(components, f64).astype(f32)
    bad = ~np.isfinite(X).all(1)
    with np.errstate(all="ignore"):
        xc = np.where(bad[:, None], f32(0), X) - m32[None, :]
        Z = chain(xc.astype(f32), v32.T.copy())
        if whiten:
            lam = np.asarray(values, f64)
            scale = (1.0 / np.sqrt(np.where(lam > 0.0, lam, 1.0))).astype(f32)
            Z = np.where(lam > 0.0, Z * scale[None, :], f32(0)).astype(f32)
    Z[bad] = np.nan
    return Z


def direct(X):
    """the independent answer: (mean, C, values descending, components as rows) by fp64 numpy and LAPACK's eigh"""
    X = np.asarray(X, f32).astype(f64)
    mean = X.mean(0)
    Xc = X - mean
    C = Xc.T @ Xc / (X.shape[0] - 1)
    w, V = np.linalg.eigh(C)
    return mean, C, w[::-1].copy(), V[:, ::-1].T.copy()
