"""numpy fp64 restatement of K23 (gae_kmeans_*), written from the contract in include/gae_hip_experimental.h: brute-force
assignment with lowest-index ties, segment means with the empty-cluster rule, shift2 / inertia / the stopping rule, and
the k-means++ seeding as an exponential race on the Philox streams.  Shared by tests/test_kmeans_cpu.py and
tests/test_gpu_kmeans.py."""
import numpy as np

from sampled_ref import philox4x32_10

M32 = 0xFFFFFFFF
KEY_XOR = 0x9E3779B97F4A7C15


def blobs(n, d, k, seed=1, noise=0.25):
    """fp32 [n, d]: centres integers(-16..16) / 4, row i around centre i mod k, noise ``noise`` N(0, 1)"""
    rng = np.random.default_rng(seed)
    centres = rng.integers(-16, 17, (k, d)) / 4.0
    return (centres[np.arange(n) % k] + noise * rng.standard_normal((n, d))).astype(np.float32)


def dist2(X, C):
    """fp64 [n, k]: |x_i - c_c|^2, taken directly"""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    out = np.empty((X.shape[0], C.shape[0]))
    for c in range(C.shape[0]):
        out[:, c] = ((X - C[c]) ** 2).sum(1)
    return out


def assign(X, C):
    """(labels int64 [n], dist2 fp64 [n], D fp64 [n, k]): argmin with the lowest index among equals"""
    D = dist2(X, C)
    labels = D.argmin(1)                       # numpy: the first minimum
    return labels, D[np.arange(D.shape[0]), labels], D


def update(X, labels, C):
    """(new centres fp64 [k, d], counts int64 [k], n_empty, shift2): segment means; a cluster without rows keeps its
    centre"""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    k = C.shape[0]
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    new = C.copy()
    for c in range(k):
        if counts[c]:
            new[c] = X[labels == c].sum(0) / counts[c]
    return new, counts, int((counts == 0).sum()), float(((new - C) ** 2).sum())


def lloyd(X, C0, tol_abs=-1.0, max_iter=100):
    """Lloyd iterations as gae_kmeans_step runs them.  Returns a dict: labels, centers, counts, inertia (of the labels
    against the centres they were chosen with), n_iter, converged, n_empty, shift2 and ``gap``: the smallest
    (second - best) / second over every row of every iteration (inf for k = 1)"""
    C = np.asarray(C0, np.float64).copy()
    labels = np.full(np.asarray(X).shape[0], -1, np.int64)
    out = {"gap": np.inf, "converged": False, "n_iter": 0}
    for it in range(max_iter):
        new_labels, d2, D = assign(X, C)
        if D.shape[1] > 1:
            two = np.partition(D, 1, axis=1)[:, :2]
            out["gap"] = min(out["gap"], float(((two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], 1e-300)).min()))
        changed = int((new_labels != labels).sum())
        labels = new_labels
        C, counts, n_empty, shift2 = update(X, labels, C)
        out.update(labels=labels, centers=C, counts=counts, inertia=float(d2.sum()), n_iter=it + 1, n_empty=n_empty,
                   shift2=shift2, changed=changed)
        if changed == 0 or shift2 <= tol_abs:
            out["converged"] = True
            break
    return out


def philox_words(ctr, draw, key):
    """word 0 of philox4x32_10(ctr, draw, key) for an int array ``ctr`` (uint64 arithmetic on 32-bit values)"""
    ctr = np.asarray(ctr, np.uint64)
    m = np.uint64(M32)
    c = [ctr & m, (ctr >> np.uint64(32)) & m, np.full_like(ctr, draw & M32), np.full_like(ctr, (draw >> 32) & M32)]
    k0, k1 = key & M32, (key >> 32) & M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)) & m, p1 & m,
             ((p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)) & m, p0 & m]
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c[0]


def seed_pp(X, k, seed):
    """(chosen int64 [k], gaps fp64 [k - 1]): the k-means++ picks of gae_kmeans_init_pp and, per round r >= 1, the
    relative gap (best - second) / best between the two largest keys (inf where fewer than two keys are positive)"""
    X = np.asarray(X, np.float64)
    n = X.shape[0]
    key = (int(seed) ^ KEY_XOR) & (2 ** 64 - 1)
    chosen = [philox4x32_10(0, 0, key)[0] % n]
    mind2 = np.full(n, np.inf)
    gaps = []
    idx = np.arange(n)
    for r in range(1, k):
        mind2 = np.minimum(mind2, ((X - X[chosen[-1]]) ** 2).sum(1))
        m = (philox_words(idx, r, key) >> np.uint64(8)).astype(np.float64)
        u = (m + 0.5) / 16777216.0
        keys = mind2 / -np.log(u)
        pick = int(np.argmax(keys))                    # numpy: the first maximum = the lowest index among equals
        top = np.sort(keys)[-2:] if n > 1 else np.array([0.0, keys[pick]])
        gaps.append((top[1] - top[0]) / top[1] if top[1] > 0 and top[0] > 0 else np.inf)
        chosen.append(pick)
    return np.asarray(chosen, np.int64), np.asarray(gaps, np.float64)


def tolerant_excess(X, C, labels):
    """per row: D64(i, label_i) - min_c D64(i, c) and the allowance 1e-5 (|x_i|^2 + max_c |c_c|^2)"""
    D = dist2(X, C)
    X64, C64 = np.asarray(X, np.float64), np.asarray(C, np.float64)
    allow = 1e-5 * ((X64 ** 2).sum(1) + (C64 ** 2).sum(1).max())
    return D[np.arange(D.shape[0]), np.asarray(labels, np.int64)] - D.min(1), allow
