"""K28 restated in numpy (tests only): multinomial logistic regression with an L2 penalty by the accelerated majoriser
iteration of include/gae_hip_experimental.h.  ``dtype`` is the arithmetic of a PASS (x~ = x - p, the logits, the
softmax, the residual, the gradient product); everything else -- the moments, the factor, the update, the restart test,
the stopping rule -- is fp64, as on the device.

A model's parameters are W [c, D1], D1 = d + 1, column 0 the intercept about the pivot p; ``to_model`` maps them to
(coef [c, d], intercept [c]) in the caller's coordinates."""
import numpy as np

LAMBDAS = [10.0 ** (e / 2.0) for e in range(-6, 7)]         # ops.logreg's default grid


def make_case(n, d, c, seed=0, sep=2.0):
    """overlapping Gaussian clusters; the features scaled by 0.5 .. 20 and shifted by up to +-30.  (X fp32, y int64)"""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(c, d)) * sep / np.sqrt(2.0 * d)      # about `sep` noise deviations apart
    y = rng.integers(0, c, n)
    Z = centres[y] + rng.normal(size=(n, d))
    scale = np.exp(rng.uniform(np.log(0.5), np.log(20.0), d))
    shift = rng.uniform(-30.0, 30.0, d)
    return (Z * scale + shift).astype(np.float32), y.astype(np.int64)


def deal_folds(n, F, seed=0, ragged=False):
    """a fold id per row: round-robin over a permutation, or (ragged) fold sizes that differ by design"""
    rng = np.random.default_rng(seed + 1000)
    if not ragged:
        fold = np.empty(n, dtype=np.int64)
        fold[rng.permutation(n)] = np.arange(n) % F
        return fold
    w = np.arange(1, F + 1, dtype=np.float64)
    return rng.choice(F, size=n, p=w / w.sum()).astype(np.int64)


def pivot_of(X, rows):
    """the fp32 column means of the listed rows (any fp32 vector near them serves: the model does not depend on it)"""
    return X[rows].astype(np.float64).mean(0).astype(np.float32)


def augmented(X, rows, pivot, dtype=np.float64):
    """x~ = [1, x - p] of the listed rows: widened to ``dtype`` first, then one rounded subtraction"""
    Xt = X[rows].astype(dtype) - np.asarray(pivot).astype(dtype)
    return np.concatenate([np.ones((len(rows), 1), dtype=dtype), Xt], 1)


def majoriser(X, rows, pivot, lam):
    """A = S / 2 + lambda diag(0, 1 .. 1), S = sum [1, x~][1, x~]^T in fp64 (Boehning's bound on the Hessian)"""
    Xa = augmented(X, rows, pivot)
    A = 0.5 * (Xa.T @ Xa)
    A[np.arange(1, A.shape[0]), np.arange(1, A.shape[0])] += lam
    return A


def softmax_rows(Z):
    """the stated order: max, subtract, exp, ascending sum, one reciprocal"""
    E = np.exp(Z - Z.max(1, keepdims=True))
    s = np.zeros(E.shape[0], dtype=E.dtype)
    for k in range(E.shape[1]):
        s = s + E[:, k]
    return E * (np.ones_like(s) / s)[:, None]


def gradient(Xa, onehot, V, lam, dtype=np.float64):
    """G = X~^T (softmax(X~ V^T) - Y) + lambda D V: the pass in ``dtype``, the sum with the penalty in fp64"""
    Vd = V.astype(dtype)
    R = softmax_rows(Xa @ Vd.T) - onehot.astype(dtype)
    G = (R.T @ Xa).astype(np.float64)
    G[:, 1:] += lam * V[:, 1:].astype(np.float64)
    return G


def fit(X, y, rows, lam, c, pivot, tol=1e-4, max_iter=1000, dtype=np.float64):
    """(W fp64 [c, D1], n_iter, converged) of the model trained on ``rows``"""
    rows = np.asarray(rows, dtype=np.int64)
    Xa = augmented(X, rows, pivot, dtype)
    onehot = np.eye(c)[y[rows]]
    Ainv = np.linalg.inv(majoriser(X, rows, pivot, lam))
    W = np.zeros((c, Xa.shape[1]))
    Wp = W.copy()
    t = 1.0
    for it in range(1, max_iter + 1):
        t1 = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
        V = (W + ((t - 1.0) / t1) * (W - Wp)).astype(dtype).astype(np.float64)           # V is stored in the pass's format
        G = gradient(Xa, onehot, V, lam, dtype)
        dV = -(G @ Ainv)
        Wn = V + dV
        t = 1.0 if float((G * (Wn - W)).sum()) > 0.0 else t1
        Wp, W = W, Wn
        if np.abs(dV).max() <= tol * max(1.0, np.abs(Wn).max()):
            return W, it, True
    return W, max_iter, False


def objective(X, y, rows, lam, pivot, W):
    """J(W) in fp64"""
    rows = np.asarray(rows, dtype=np.int64)
    Z = augmented(X, rows, pivot) @ W.T
    mx = Z.max(1)
    nll = np.log(np.exp(Z - mx[:, None]).sum(1)) + mx - Z[np.arange(len(rows)), y[rows]]
    return float(nll.sum() + 0.5 * lam * (W[:, 1:] ** 2).sum())


def majoriser_step(X, y, rows, lam, pivot, W):
    """max |A^-1 G(W)| with the exact (fp64) gradient: how far one more step would move"""
    rows = np.asarray(rows, dtype=np.int64)
    G = gradient(augmented(X, rows, pivot), np.eye(W.shape[0])[y[rows]], W, lam)
    return float(np.abs(np.linalg.solve(majoriser(X, rows, pivot, lam), G.T)).max())


def to_model(W, pivot):
    """(coef [c, d], intercept [c]): b = W[:, 0] - W[:, 1:] p"""
    return W[:, 1:].copy(), W[:, 0] - W[:, 1:] @ np.asarray(pivot, dtype=np.float64)


def from_model(coef, intercept, pivot):
    """W [c, D1] about the pivot of a model in the caller's coordinates"""
    p = np.asarray(pivot, dtype=np.float64)
    return np.concatenate([(intercept + coef @ p)[:, None], coef], 1)


def heldout(X, y, rows, coef, intercept, margin=1e-4):
    """(nll, correct, kept, n): fp64 negative log-likelihood over ``rows``; the arg-max count over the rows whose top two
    logits are at least ``margin`` apart (``kept``: which)"""
    rows = np.asarray(rows, dtype=np.int64)
    Z = X[rows].astype(np.float64) @ coef.T + intercept
    mx = Z.max(1)
    nll = np.log(np.exp(Z - mx[:, None]).sum(1)) + mx - Z[np.arange(len(rows)), y[rows]]
    top = np.sort(Z, 1)
    kept = top[:, -1] - top[:, -2] >= margin
    hit = Z.argmax(1) == y[rows]
    return float(nll.sum()), hit, kept
