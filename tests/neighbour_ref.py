"""numpy restatement of K35 / K36 (gae_neighbour_pairs, gae_neighbour_topk), written from the contract comment of
include/gae_hip_experimental.h: Gamma(i) as the distinct non-self columns, the dense int64 route A diag(w) A for the sums,
the same fixed-point weight tables from the same numpy calls, the candidate rule and the (value descending, j ascending)
order.  O(n^2) memory and O(n^3) integer work -- test sizes only; nothing here is on a product path."""
import numpy as np

SCALE_BITS = 32
KINDS = ("cn", "jaccard", "aa", "ra")


def random_graph(n, u, seed):
    """the generator of the tests: u undirected pairs, a == b dropped, the first 20 pairs again as duplicates, 5 self-loops,
    both directions listed.  Returns (src, dst) int64."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n, u)
    b = rng.integers(0, n, u)
    keep = a != b
    a, b = a[keep], b[keep]
    a, b = np.concatenate([a, a[:20]]), np.concatenate([b, b[:20]])
    loops = rng.integers(0, n, 5)
    a, b = np.concatenate([a, loops]), np.concatenate([b, loops])
    return np.concatenate([a, b]).astype(np.int64), np.concatenate([b, a]).astype(np.int64)


def adjacency(n, src, dst):
    """bool [n, n]: A[i, j] is j in Gamma(i) -- duplicates once, the diagonal empty"""
    A = np.zeros((n, n), dtype=bool)
    A[np.asarray(dst, np.int64), np.asarray(src, np.int64)] = True
    A[np.arange(n), np.arange(n)] = False
    return A


def weight_table(max_degree):
    """int64 [max_degree + 1, 2]: aa_q[d] = rint(2^32 / log(d)) for d >= 2, ra_q[d] = rint(2^32 / d) for d >= 1, else 0"""
    d = np.arange(int(max_degree) + 1, dtype=np.float64)
    scale = np.float64(2.0) ** SCALE_BITS
    table = np.zeros((d.shape[0], 2), dtype=np.int64)
    table[2:, 0] = np.rint(scale / np.log(d[2:])).astype(np.int64)
    table[1:, 1] = np.rint(scale / d[1:]).astype(np.int64)
    return table


def weights(A):
    """(deg int64 [n], W int64 [n, 2]) of an adjacency"""
    deg = A.sum(1).astype(np.int64)
    return deg, weight_table(int(deg.max()) if deg.size else 0)[deg]


def pair_scores(A, pairs, chunk=4096):
    """dict of the NeighbourScores fields for pairs int [2, m]"""
    deg, W = weights(A)
    pi, pj = np.asarray(pairs[0], np.int64), np.asarray(pairs[1], np.int64)
    m = pi.shape[0]
    common = np.zeros(m, np.int64)
    wsum = np.zeros((m, 2), np.int64)
    for s in range(0, m, chunk):
        both = A[pi[s:s + chunk]] & A[pj[s:s + chunk]]
        common[s:s + chunk] = both.sum(1)
        wsum[s:s + chunk] = both.astype(np.int64) @ W
    deg_i, deg_j = deg[pi], deg[pj]
    union = deg_i + deg_j - common
    jaccard = np.zeros(m, np.float64)
    nz = union > 0
    jaccard[nz] = common[nz].astype(np.float64) / union[nz].astype(np.float64)
    inv = np.float64(2.0) ** -SCALE_BITS
    return {"common": common, "deg_i": deg_i, "deg_j": deg_j, "union": union, "cn": common, "jaccard": jaccard,
            "aa": wsum[:, 0].astype(np.float64) * inv, "ra": wsum[:, 1].astype(np.float64) * inv, "pa": deg_i * deg_j,
            "aa_sum": wsum[:, 0].copy(), "ra_sum": wsum[:, 1].copy()}


def two_hop(A, rows, kind):
    """(common int64 [m, n], wsum int64 [m, n]) of the query rows: rows of A A and of A diag(w) A"""
    deg, W = weights(A)
    Ai = A.astype(np.int64)
    common = Ai[rows] @ Ai
    col = {"aa": 0, "ra": 1}.get(kind)
    wsum = np.zeros_like(common) if col is None else Ai[rows] @ (Ai * W[:, col][:, None])
    return common, wsum


def topk(A, k, kind, exclude_edges=True, rows=None):
    """(index int32 [m, k], value fp64 [m, k], common int32 [m, k]) and the candidate count of every query row"""
    assert kind in KINDS
    n = A.shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    m = rows.shape[0]
    deg, _ = weights(A)
    common, wsum = two_hop(A, rows, kind)
    cand = common >= 1
    cand[np.arange(m), rows] = False
    if exclude_edges:
        cand &= ~A[rows]
    inv = np.float64(2.0) ** -SCALE_BITS
    if kind == "cn":
        key, value = common, common.astype(np.float64)
    elif kind == "jaccard":
        union = deg[rows][:, None] + deg[None, :] - common
        value = common.astype(np.float64) / np.maximum(union, 1).astype(np.float64)
        key = value
    else:
        key, value = wsum, wsum.astype(np.float64) * inv
    index = np.full((m, k), -1, np.int32)
    out_v = np.full((m, k), -np.inf, np.float64)
    out_c = np.zeros((m, k), np.int32)
    for r in range(m):
        js = np.flatnonzero(cand[r])
        order = js[np.lexsort((js, -key[r, js]))][:k]          # larger key first, then lower j
        index[r, :order.size] = order
        out_v[r, :order.size] = value[r, order]
        out_c[r, :order.size] = common[r, order]
    return index, out_v, out_c, cand.sum(1)


def tied_rows(A, k, kind, exclude_edges=True):
    """rows with more than k candidates whose k-th and (k + 1)-th keys are equal: the order by j decides their list"""
    index, value, _, count = topk(A, k + 1, kind, exclude_edges)
    full = count > k
    return np.flatnonzero(full & (value[:, k - 1] == value[:, k]))
