"""K25 restated in numpy fp64 (tests only).  Two routes to the same numbers:

``moments`` + ``solve`` mirror the C ABI (gae_ridge_stats / gae_ridge_solve, include/gae_hip_experimental.h): per-fold
second moments of v = [1, x - p_x, y - p_y] as packed upper triangles, then every (model, lambda) cell from the moments
alone -- centring, Cholesky, the intercept mapped back through the pivot, the held-out SSE as u^T M_m u.

``direct`` does not use moments: for every fold and lambda it centres the training rows, solves the augmented least
squares problem [X_c ; sqrt(lambda) I] w = [y_c ; 0] with np.linalg.lstsq, and takes the held-out residuals row by row."""
import numpy as np

NO_INTERCEPT = 1
LAMBDAS = [10.0 ** (e / 2.0) for e in range(-6, 7)]         # ops.ridge's default grid


def tri(w):
    return w * (w + 1) // 2


def pack_upper(M):
    return M[np.triu_indices(M.shape[0])]


def unpack_upper(p, W):
    M = np.zeros((W, W))
    M[np.triu_indices(W)] = p
    return M + np.triu(M, 1).T


def fold_lists(fold, F):
    """(rows int32, fold_ptr int32 [F + 1]): the rows stably sorted by fold, -1 dropped"""
    fold = np.asarray(fold)
    rows = np.concatenate([np.flatnonzero(fold == f) for f in range(F)]).astype(np.int32)
    counts = np.array([(fold == f).sum() for f in range(F)])
    return rows, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def moments(X, Y, rows, fold_ptr, pivot=None):
    """stats fp64 [F, W (W + 1) / 2]; rows = None: all rows in one fold"""
    X, Y = np.asarray(X), np.asarray(Y)
    Y = Y.reshape(Y.shape[0], -1)
    d, t = X.shape[1], Y.shape[1]
    if rows is None:
        rows, fold_ptr = np.arange(X.shape[0]), np.array([0, X.shape[0]])
    p = np.zeros(d + t) if pivot is None else np.asarray(pivot, dtype=np.float64)
    out = []
    for f in range(len(fold_ptr) - 1):
        r = np.asarray(rows[fold_ptr[f]:fold_ptr[f + 1]], dtype=np.int64)
        V = np.concatenate([np.ones((len(r), 1)), X[r].astype(np.float64) - p[:d], Y[r].astype(np.float64) - p[d:]], 1)
        out.append(pack_upper(V.T @ V))
    return np.stack(out)


def solve(stats, d, t, lambdas, pivot=None, flags=0):
    """(coef [F + 1, L, t, d], intercept [F + 1, L, t], cv_sse [F, L, t], info int32 [F + 1, L]) from the moments"""
    F, L, W = stats.shape[0], len(lambdas), 1 + d + t
    p = np.zeros(d + t) if pivot is None else np.asarray(pivot, dtype=np.float64)
    M = [unpack_upper(stats[f], W) for f in range(F)]
    coef = np.full((F + 1, L, t, d), np.nan)
    icpt = np.full((F + 1, L, t), np.nan)
    sse = np.full((F, L, t), np.nan)
    info = np.zeros((F + 1, L), dtype=np.int32)
    for m in range(F + 1):
        S = np.zeros((W, W))
        for f in range(F):
            if f != m:
                S = S + M[f]
        c = S[0, 0]
        for l, lam in enumerate(lambdas):
            if not (lam >= 0 and np.isfinite(lam)):
                info[m, l] = -2
                continue
            if not c > 0:
                info[m, l] = -1
                continue
            if flags & NO_INTERCEPT:
                mu = np.zeros(d + t)
                C = S[1:, 1:] + np.outer(p, S[0, 1:]) + np.outer(S[0, 1:], p) + c * np.outer(p, p)
            else:
                mu = S[0, 1:] / c
                C = S[1:, 1:] - np.outer(S[0, 1:], mu)
            A = C[:d, :d] + lam * np.eye(d)
            Lc = np.zeros((d, d))
            for j in range(d):                                         # Cholesky by columns, LAPACK's info
                piv = A[j, j] - Lc[j, :j] @ Lc[j, :j]
                if not (piv > 0 and np.isfinite(piv)):
                    info[m, l] = j + 1
                    break
                Lc[j, j] = np.sqrt(piv)
                Lc[j + 1:, j] = (A[j + 1:, j] - Lc[j + 1:, :j] @ Lc[j, :j]) / Lc[j, j]
            if info[m, l]:
                continue
            z = np.zeros((d, t))
            for i in range(d):                                         # forward: L z = C_xy
                z[i] = (C[i, d:] - Lc[i, :i] @ z[:i]) / Lc[i, i]
            w = np.zeros((d, t))
            for i in range(d - 1, -1, -1):                             # back: L^T w = z
                w[i] = (z[i] - Lc[i + 1:, i] @ w[i + 1:]) / Lc[i, i]
            w = w.T                                                    # [t, d]
            if flags & NO_INTERCEPT:
                b = np.zeros(t)
                bq = w @ p[:d] - p[d:]
            else:
                bq = mu[d:] - w @ mu[:d]
                b = p[d:] + mu[d:] - w @ mu[:d] - w @ p[:d]
            coef[m, l], icpt[m, l] = w, b
            if m < F:
                for j in range(t):
                    u = np.zeros(W)
                    u[0], u[1:1 + d], u[1 + d + j] = -bq[j], -w[j], 1.0
                    sse[m, l, j] = u @ M[m] @ u
    return coef, icpt, sse, info


def direct(X, Y, fold, lambdas, fit_intercept=True):
    """the same tables without moments; ``fold`` int [n] with values in -1 .. F - 1.  Returns (coef, intercept, cv_sse,
    cond [F + 1, L]: np.linalg.cond of C_xx + lambda I of every cell)"""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64).reshape(X.shape[0], -1)
    fold = np.asarray(fold)
    F, L, d, t = int(fold.max()) + 1, len(lambdas), X.shape[1], Y.shape[1]
    coef = np.zeros((F + 1, L, t, d))
    icpt = np.zeros((F + 1, L, t))
    sse = np.zeros((F, L, t))
    cond = np.zeros((F + 1, L))
    for m in range(F + 1):
        tr = (fold >= 0) & (fold != m)
        mx = X[tr].mean(0) if fit_intercept else np.zeros(d)
        my = Y[tr].mean(0) if fit_intercept else np.zeros(t)
        Xc, Yc = X[tr] - mx, Y[tr] - my
        for l, lam in enumerate(lambdas):
            A = np.concatenate([Xc, np.sqrt(lam) * np.eye(d)])
            B = np.concatenate([Yc, np.zeros((d, t))])
            w = np.linalg.lstsq(A, B, rcond=None)[0].T                 # [t, d]
            b = my - w @ mx
            coef[m, l], icpt[m, l] = w, b
            cond[m, l] = np.linalg.cond(Xc.T @ Xc + lam * np.eye(d))
            if m < F:
                ho = fold == m
                r = Y[ho] - (X[ho] @ w.T + b)
                sse[m, l] = (r * r).sum(0)
    return coef, icpt, sse, cond


# ------------------------------------------------------------------ shared by the CPU and the GPU tests
def make_case(n, d, t, F, offset=0.0, seed=0):
    """standard normal features (plus a common offset), targets linear in them plus noise; a permutation dealt
    round-robin into F folds"""
    rng = np.random.default_rng(seed)
    X = (rng.standard_normal((n, d)) + offset).astype(np.float32)
    w = rng.standard_normal((d, t))
    Y = (X.astype(np.float64) @ w / np.sqrt(d) + 0.3 * rng.standard_normal((n, t)) + 2.0).astype(np.float32)
    return X, Y, rng.permutation(n) % F


def bound_of(X, Y, fold, F, pivot, cond):
    """64 d kappa (1 + rho^2) 2^-53 per (model, lambda); rho = max over folds and columns of |mean_f - pivot| / std_f"""
    Z = np.concatenate([X, Y], 1).astype(np.float64)
    p = np.zeros(Z.shape[1]) if pivot is None else np.asarray(pivot, dtype=np.float64)
    rho = max((np.abs(Z[fold == f].mean(0) - p) / Z[fold == f].std(0)).max() for f in range(F))
    return 64 * X.shape[1] * cond * (1 + rho ** 2) * 2.0 ** -53


def errors_over_bound(got, want, sst, bound, X, Y):
    """max over the cells of |dw|_inf / |w|_inf / bound, of |dSSE| / SST / bound and of |db| over its limit.  The
    intercept b = mean_y - mean_x . w inherits the error of w through the column means, plus the rounding of its own
    d + 2 terms: |db| <= (bound + 4 d eps) |w|_inf |mean_x|_1 + 4 d eps (1 + |mean_y|_inf)"""
    coef, icpt, sse = got
    coef2, icpt2, sse2 = want
    F, d, eps = sse2.shape[0], coef2.shape[3], 2.0 ** -53
    wmax = np.abs(coef2).max((2, 3))
    ew = np.abs(coef - coef2).max((2, 3)) / wmax
    es = (np.abs(sse - sse2) / sst).max(2)
    mx, my = np.abs(np.asarray(X, dtype=np.float64).mean(0)).sum(), np.abs(np.asarray(Y, dtype=np.float64).mean(0)).max()
    limit = (bound + 4 * d * eps) * wmax * mx + 4 * d * eps * (1 + my)
    eb = np.abs(icpt - icpt2).max(2) / limit
    return float((ew / bound).max()), float((es / bound[:F]).max()), float(eb.max())
