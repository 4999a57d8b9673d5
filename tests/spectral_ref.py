"""numpy restatement of K32 (gae_spectral_*, ops.spectral_embedding), written from the K32 comment of
include/gae_hip_experimental.h: the scales, the Philox words of the start block, the operator product as one fp64 fma chain
per element in CSR order, the small solve step by step (Cholesky-Crout, the two triangular reductions, K31's Jacobi
through tests/pca_ref.py on the packed triangle, the back substitution), the filter's coefficients, the rotation's chains,
the residual partials and their fold, the sign rule and the scalings.  The device must return the same bits for each of
these from the same inputs; only the Gram pair (a different order of the same sums) and the start block's library
functions are compared within bounds.  ``dense`` / ``lapack`` are the independent answer.  Shared by
tests/test_spectral_cpu.py and tests/test_gpu_spectral.py; no kernel code is imported."""
import collections
import functools

import numpy as np

import noise_ref
import pca_ref

f32, f64 = np.float32, np.float64
MAX_B, MAX_K, MAX_DEGREE, CHUNK = 128, 64, 12, 256
KEY_XOR = 0x5851F42D4C957F2D
FLOOR, LOWEST = 0.02, -0.5

Case = collections.namedtuple("Case", ["name", "kind", "n", "k", "oversample", "self_loops"])
Graph = collections.namedtuple("Graph", ["n", "indptr", "indices", "src", "dst", "labels"])
Solved = collections.namedtuple("Solved", ["T", "values", "coef", "info", "L", "Hp", "W"])
Run = collections.namedtuple("Run", ["vectors", "embedding", "values", "residuals", "n_iter", "n_spmm", "converged", "info",
                                     "V", "s"])

# The smallest shapes at which the kernels can go wrong: b = 2, 16, 18, 128 (both sides of the 16-wide tile edges), n = 255,
# 256, 257 (both sides of the 256-row chunk), a hub row longer than any lane group, rows with s_i = 0, the repeated
# eigenvalue 1 of a disconnected graph (the case that needs the floor under the filter's interval), self loops on and off,
# duplicate edges, rows of odd length (a CSR row that starts off a 16-byte boundary).
CASES = [
    Case("cycle64", "cycle", 64, 5, 9, False),
    Case("cliques_b2", "cliques", 15, 1, 1, False),
    Case("cliques_loops", "cliques", 15, 2, 8, True),
    Case("star300", "star", 300, 2, 14, False),
    Case("n257_b18", "random", 257, 9, 9, False),
    Case("n255_b128", "random", 255, 64, 64, False),
    Case("n256_loops", "random", 256, 8, 8, True),
    Case("multi100", "multi", 100, 4, 8, False),
    Case("planted700", "planted", 700, 8, 8, False),
    Case("sbm2708", "sbm", 2708, 16, 16, False),
]
BY_NAME = {c.name: c for c in CASES}
N_CLASSES = 7


def width(case):
    return case.k + case.oversample


# ------------------------------------------------------------------ graphs
def _csr(n, src, dst):
    """(indptr, indices) int32 of the edge list, rows = dst, columns ascending inside a row (duplicates kept): the order
    of graph.csr()"""
    order = np.lexsort((src, dst))
    indptr = np.zeros(n + 1, np.int64)
    np.add.at(indptr, dst + 1, 1)
    return np.cumsum(indptr).astype(np.int32), src[order].astype(np.int32)


def _sym(u, v):
    return np.concatenate([u, v]), np.concatenate([v, u])


@functools.lru_cache(maxsize=None)
def graph(name):
    """the case's symmetric graph (both directions of every edge listed)"""
    case = BY_NAME[name]
    n, kind = case.n, case.kind
    rng = np.random.default_rng(sum(name.encode()) * 7919 + n)
    labels = None
    if kind == "cycle":
        u = np.arange(n)
        src, dst = _sym(u, (u + 1) % n)
    elif kind == "cliques":                                             # 5 + 7 nodes, three isolated ones
        pairs = [(i, j) for lo, hi in ((0, 5), (5, 12)) for i in range(lo, hi) for j in range(i + 1, hi)]
        src, dst = _sym(*np.array(pairs).T)
    elif kind == "star":
        src, dst = _sym(np.zeros(n - 1, np.int64), np.arange(1, n))
    elif kind in ("random", "multi"):
        m = 4 * n
        u, v = rng.integers(0, n, m), rng.integers(0, n, m)
        keep = u != v
        key = np.unique(np.minimum(u, v)[keep] * n + np.maximum(u, v)[keep])
        u, v = key // n, key % n
        if kind == "multi":                                            # every fifth edge twice, every 25th three times
            u = np.concatenate([u, u[::5], u[::25]])
            v = np.concatenate([v, v[::5], v[::25]])
        src, dst = _sym(u, v)
    else:
        # planted classes.  "planted": one block model.  "sbm": a block model on the first 2400 nodes, the rest in 154
        # components of two nodes (Cora's shape: a giant component and many tiny ones, the top eigenvalue 1 repeated)
        core = n if kind == "planted" else 2400
        labels = rng.integers(0, N_CLASSES, n)
        d_in, d_out = (10.0, 2.0) if kind == "planted" else (3.2, 0.8)  # expected neighbours inside / outside the class
        iu, ju = np.triu_indices(core, 1)
        p = np.where(labels[iu] == labels[ju], d_in * N_CLASSES / core, d_out * N_CLASSES / (6.0 * core))
        on = rng.random(iu.shape[0]) < p
        u, v = iu[on], ju[on]
        if core < n:
            extra = np.arange(core, n - (n - core) % 2).reshape(-1, 2)
            labels[extra[:, 1]] = labels[extra[:, 0]]
            u, v = np.concatenate([u, extra[:, 0]]), np.concatenate([v, extra[:, 1]])
        src, dst = _sym(u, v)
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    indptr, indices = _csr(n, src, dst)
    return Graph(n, indptr, indices, src, dst, labels)


def dense(g, sigma):
    """the dense S = D^-1/2 (A + sigma I) D^-1/2 in plain fp64 (duplicates counted)"""
    A = np.zeros((g.n, g.n), f64)
    np.add.at(A, (g.dst, g.src), 1.0)
    deg = A.sum(1) + sigma
    with np.errstate(divide="ignore"):
        s = np.where(deg > 0, 1.0 / np.sqrt(deg), 0.0)
    return s[:, None] * (A + sigma * np.eye(g.n)) * s[None, :]


@functools.lru_cache(maxsize=None)
def lapack(name):
    """(values descending, vectors as columns) of the case's dense S by LAPACK's eigh"""
    case = BY_NAME[name]
    w, U = np.linalg.eigh(dense(graph(name), 1.0 if case.self_loops else 0.0))
    return w[::-1].copy(), U[:, ::-1].copy()


# ------------------------------------------------------------------ fp64 fma
def _two_sum(a, b):
    s = a + b
    t = s - a
    return s, (a - (s - t)) + (b - t)


def fma64(a, b, c):
    """fp64 fma(a, b, c) exactly (Boldo & Melquiond's emulation): the product as an error-free pair (Veltkamp / Dekker),
    an error-free sum of c and its high part, the two low parts added with rounding to odd, one final rounding.  Exact
    short of overflow and of products below 2^-969."""
    a, b, c = np.broadcast_arrays(np.asarray(a, f64), np.asarray(b, f64), np.asarray(c, f64))
    with np.errstate(all="ignore"):
        p = a * b
        t = 134217729.0 * a
        ah = t - (t - a)
        al = a - ah
        t = 134217729.0 * b
        bh = t - (t - b)
        bl = b - bh
        pl = ((ah * bh - p) + ah * bl + al * bh) + al * bl
        th, tl = _two_sum(c, p)
        v, err = _two_sum(tl, pl)
        v = np.ascontiguousarray(v)
        even = (v.view(np.int64) & 1) == 0
        fix = np.isfinite(v) & (err != 0) & even
        v = np.where(fix, np.nextafter(v, np.where(err > 0, np.inf, -np.inf)), v)
        return th + v


# ------------------------------------------------------------------ set-up
def scale(indptr, sigma):
    deg = np.diff(np.asarray(indptr, np.int64)).astype(f64) + f64(sigma)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(deg > 0.0, 1.0 / np.sqrt(deg), 0.0)


def init_uniforms(n, b, seed):
    """(u1, u2) fp64 [n b]: exact"""
    total = n * b
    nq = (total + 3) // 4
    w = noise_ref.philox_words(np.arange(nq, dtype=np.uint64), 0, 0, (int(seed) ^ KEY_XOR) & 0xFFFFFFFFFFFFFFFF)
    u1 = ((w[:, 0::2] >> np.uint32(8)).astype(f64) + 0.5) * 2.0 ** -24
    u2 = (w[:, 1::2] >> np.uint32(8)).astype(f64) * 2.0 ** -24
    return np.repeat(u1.reshape(-1), 2)[:total], np.repeat(u2.reshape(-1), 2)[:total]


def init(n, b, seed):
    """(V [n, b], rad [n, b]): the start block with numpy's log / cos / sin"""
    u1, u2 = init_uniforms(n, b, seed)
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = 6.283185307179586 * u2
    odd = (np.arange(n * b) & 1) == 1
    return (rad * np.where(odd, np.sin(ang), np.cos(ang))).reshape(n, b), rad.reshape(n, b)


# ------------------------------------------------------------------ the operator product
def spmm(indptr, indices, s, sigma, Yin, Yprev, coef):
    """Yout of gae_spectral_spmm: the chain of every element, neighbours in CSR order"""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    n, b = Yin.shape
    alpha, beta, gamma = (f64(x) for x in coef)
    deg = np.diff(indptr)
    acc = np.zeros((n, b), f64)
    for p in range(int(deg.max()) if n else 0):
        rows = np.nonzero(deg > p)[0]
        j = indices[indptr[rows] + p]
        acc[rows] = fma64(s[j][:, None], Yin[j], acc[rows])
    if sigma != 0.0:
        acc = fma64((f64(sigma) * s)[:, None], Yin, acc)
    with np.errstate(all="ignore"):
        t = s[:, None] * acc
        o = fma64(beta, Yin, alpha * t)
        if Yprev is not None:
            o = fma64(gamma, Yprev, o)
    return o


# ------------------------------------------------------------------ Gram pair
def gram(V, AV):
    """(G, H) full symmetric from the upper triangles of the plain fp64 products (the device adds the same terms in
    chunks: compared within gram_bound)"""
    G, H = V.T @ V, V.T @ AV
    return np.triu(G) + np.triu(G, 1).T, np.triu(H) + np.triu(H, 1).T


def gram_bound(V, AV):
    """gamma_n sum |v| |w| per entry, gamma_n = n u / (1 - n u), u = 2^-53"""
    n = V.shape[0]
    gam = n * 2.0 ** -53 / (1.0 - n * 2.0 ** -53)
    return gam * (np.abs(V).T @ np.abs(V)), gam * (np.abs(V).T @ np.abs(AV))


def sum_partials(parts):
    """the library's one order for a list of partial sums [P, ...] (common.h)"""
    P = parts.shape[0]
    if P <= 32:
        g = np.zeros(parts.shape[1:], f64)
        for q in range(P):
            g = g + parts[q]
        return g
    lanes = np.zeros((64,) + parts.shape[1:], f64)
    for q in range(P):
        lanes[q % 64] = lanes[q % 64] + parts[q]
    for off in (32, 16, 8, 4, 2, 1):
        lanes[:64 - off] = lanes[:64 - off] + lanes[off:].copy()
    return lanes[0]


# ------------------------------------------------------------------ the small solve
def cholesky(G):
    """(L with its diagonal, info): Cholesky-Crout column by column, k ascending, each product subtracted as formed"""
    b = G.shape[0]
    L = np.zeros((b, b), f64)
    with np.errstate(all="ignore"):
        for j in range(b):
            piv = G[j, j]
            col = G[j + 1:, j].copy()
            for k in range(j):
                piv = piv - L[j, k] * L[j, k]
                col = col - L[j + 1:, k] * L[j, k]
            if not (piv > 0.0 and piv <= np.finfo(f64).max):
                return L, j + 1
            L[j, j] = np.sqrt(piv)
            L[j + 1:, j] = col / L[j, j]
    return L, 0


def reduce_h(L, H):
    """H' = L^-1 H L^-T, the upper triangle computed and mirrored"""
    b = L.shape[0]
    X = np.zeros((b, b), f64)
    for i in range(b):
        x = H[i, :].copy()
        for k in range(i):
            x = x - L[i, k] * X[k, :]
        X[i, :] = x / L[i, i]
    Y = np.zeros((b, b), f64)
    for j in range(b):
        y = X[:, j].copy()
        for k in range(j):
            y = y - L[j, k] * Y[:, k]
        Y[:, j] = y / L[j, j]
    return np.triu(Y) + np.triu(Y, 1).T


def pack(Hp):
    """the packed triangle of width 1 + b that K31's centring returns Hp from: S[0][0] = 2, S[0][1..] = 0, S_xx = Hp"""
    b = Hp.shape[0]
    M = np.zeros((1 + b, 1 + b), f64)
    M[0, 0] = 2.0
    M[1:, 1:] = Hp
    return M[np.triu_indices(1 + b)]


def coefficients(theta, k, degree):
    b = theta.shape[0]
    coef = np.zeros((MAX_DEGREE + 1, 3), f64)
    t1, tk, tb = theta[0], theta[k - 1], theta[b - 1]
    lim = max(min(tb, tk - FLOOR), LOWEST)
    e, c = (lim + 1.0) * 0.5, (lim - 1.0) * 0.5
    s1 = e / (t1 - c)
    coef[0] = (1.0, 0.0, 0.0)
    alpha = s1 / e
    coef[1] = (alpha, -(c * alpha), 0.0)
    s = s1
    for d in range(2, degree + 1):
        s2 = 1.0 / (2.0 / s1 - s)
        alpha = (2.0 * s2) / e
        coef[d] = (alpha, -(c * alpha), -(s * s2))
        s = s2
    return coef


def solve(G, H, k, degree):
    """what gae_spectral_solve writes: T, values (theta), coef [13, 3] (rows past degree zero), info"""
    b = G.shape[0]
    nanT, nanv = np.full((b, b), np.nan), np.full(b, np.nan)
    L, info = cholesky(G)
    if info:
        return Solved(nanT, nanv, None, info, L, None, None)
    Hp = reduce_h(L, H)
    jac = pca_ref.solve(pack(Hp), b, 0, None, b)
    if jac.info != 0:
        return Solved(nanT, nanv, None, -1, L, Hp, None)
    theta, W = jac.values, jac.components
    if not np.isfinite(theta).all():
        return Solved(nanT, nanv, None, -2, L, Hp, W)
    T = np.zeros((b, b), f64)
    for i in range(b - 1, -1, -1):
        x = W[:, i].copy()
        for kk in range(i + 1, b):
            x = x - L[kk, i] * T[kk, :]
        T[i, :] = x / L[i, i]
    return Solved(T, theta, coefficients(theta, k, degree), 0, L, Hp, W)


# ------------------------------------------------------------------ rotate, residuals
def chain(X, T):
    out = np.zeros((X.shape[0], T.shape[1]), f64)
    for j in range(T.shape[0]):
        out = fma64(X[:, j:j + 1], T[j:j + 1, :], out)
    return out


def rotate(V, AV, T, theta, tol, k):
    """(V', AV', residuals [b], n_converged)"""
    n, b = V.shape
    V2, AV2 = chain(V, T), chain(AV, T)
    with np.errstate(all="ignore"):
        d = AV2 - theta[None, :] * V2
        dd = d * d
    chunks = (n + CHUNK - 1) // CHUNK
    pad = np.zeros((chunks * CHUNK, b), f64)
    pad[:n] = dd
    pad = pad.reshape(chunks, CHUNK, b)
    parts = np.zeros((chunks, b), f64)
    for r in range(CHUNK):
        parts = parts + pad[:, r, :]
    res = np.sqrt(sum_partials(parts))
    conv = 0
    while conv < k and res[conv] <= tol:
        conv += 1
    return V2, AV2, res, conv


# ------------------------------------------------------------------ finish
def finish(V, first, k, theta, s, scaling):
    """(vectors fp64 [n, k], embedding fp32 [n, k])"""
    X = V[:, first:first + k].copy()
    at = np.argmax(np.abs(X), axis=0)                                   # the first of equal magnitudes
    sign = np.where(X[at, np.arange(k)] < 0.0, -1.0, 1.0)
    X = sign[None, :] * X
    if scaling == "degree":
        Z = X * s[:, None]
    elif scaling == "value":
        Z = X * np.sqrt(np.maximum(theta[first:first + k], 0.0))[None, :]
    else:
        Z = X
    return X, Z.astype(f32)


# ------------------------------------------------------------------ the whole method
def run(name, tol=1e-8, max_iter=200, degree=8, seed=0, scaling="none", V0=None, gram_fn=gram):
    """ops.spectral_embedding on a case, launch for launch"""
    case = BY_NAME[name]
    g = graph(name)
    b, k = width(case), case.k
    sigma = 1.0 if case.self_loops else 0.0
    s = scale(g.indptr, sigma)
    V = init(g.n, b, seed)[0] if V0 is None else V0.copy()
    plain = (1.0, 0.0, 0.0)
    n_spmm, n_iter, conv, theta, res = 0, 0, 0, None, None
    for it in range(1, max_iter + 1):
        AV = spmm(g.indptr, g.indices, s, sigma, V, None, plain)
        n_spmm += 1
        G, H = gram_fn(V, AV)
        sol = solve(G, H, k, degree)
        n_iter = it
        if sol.info != 0:
            return Run(None, None, sol.values, None, n_iter, n_spmm, False, sol.info, V, s)
        theta = sol.values
        V, AV, res, conv = rotate(V, AV, sol.T, theta, tol, k)
        if conv >= k or it == max_iter:
            break
        prev, cur = None, V
        for d in range(1, degree + 1):
            nxt = spmm(g.indptr, g.indices, s, sigma, cur, prev, sol.coef[d])
            n_spmm += 1
            prev, cur = cur, nxt
        V = cur
    vec, emb = finish(V, 0, k, theta, s, scaling)
    return Run(vec, emb, theta[:k].copy(), res[:k].copy(), n_iter, n_spmm, conv >= k, 0, V, s)


@functools.lru_cache(maxsize=None)
def run_default(name):
    """the restatement's run of a case at the defaults (shared by the tests; do not modify the arrays)"""
    return run(name)


# ------------------------------------------------------------------ the conditions both test files check
def clusters(w, k, rel=1e-6):
    """[(lo, hi, delta)]: the groups of the top-k eigenvalues of a LAPACK spectrum w (descending) that lie within `rel` of
    their neighbours, each with its gap delta to the rest of the spectrum; a group cut by k is left out"""
    out, lo = [], 0
    n = w.shape[0]
    while lo < k:
        hi = lo + 1
        while hi < n and w[hi - 1] - w[hi] <= rel:
            hi += 1
        if hi <= k:
            above = w[lo - 1] - w[lo] if lo > 0 else np.inf
            below = w[hi - 1] - w[hi] if hi < n else np.inf
            out.append((lo, hi, min(above, below)))
        lo = hi
    return out


def check_result(name, vectors, values, residuals, S=None):
    """the residual, eigenvalue, projector and defect conditions on a converged result; returns the orthogonality defect.
    (1) every reported residual is the residual recomputed in plain fp64, within the rounding of that recomputation;
    (2) value c lies within its residual (plus the defect's share) of LAPACK's value of the same rank: the symmetric
        residual bound for a basis that is orthonormal up to the defect;
    (3) Davis-Kahan: for a cluster with gap delta, ||P - P_lapack||_F <= sqrt(2) (sqrt(sum res^2) / delta + defect)."""
    case = BY_NAME[name]
    g = graph(name)
    if S is None:
        S = dense(g, 1.0 if case.self_loops else 0.0)
    w, U = lapack(name)
    k = case.k
    X = np.asarray(vectors, f64)
    R = S @ X - X * values[None, :]
    rec = np.sqrt((R * R).sum(0))
    slack = 64 * g.n * 2.0 ** -53
    assert np.all(np.abs(rec - residuals) <= slack), (name, rec, residuals)
    defect = float(np.linalg.norm(X.T @ X - np.eye(k)))
    assert np.all(np.abs(values - w[:k]) <= rec + 2.0 * defect + slack), (name, values - w[:k], rec)
    for lo, hi, delta in clusters(w, k):
        P = X[:, lo:hi] @ X[:, lo:hi].T
        Q = U[:, lo:hi] @ U[:, lo:hi].T
        bound = np.sqrt(2.0) * (np.sqrt((rec[lo:hi] ** 2).sum()) / delta + defect) + slack
        assert np.linalg.norm(P - Q) <= bound, (name, lo, hi, delta, np.linalg.norm(P - Q), bound)
    return defect


def qr_defect(name):
    """||Q^T Q - I||_F of numpy.linalg.qr of a random block of the case's shape [n, k]: the yardstick of the defect"""
    case = BY_NAME[name]
    rng = np.random.default_rng(case.n + case.k)
    Q, _ = np.linalg.qr(rng.standard_normal((case.n, case.k)))
    return float(np.linalg.norm(Q.T @ Q - np.eye(case.k)))
