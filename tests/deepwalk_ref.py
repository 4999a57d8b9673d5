"""numpy restatement of K37 / K38 (gae_random_walks, gae_sgns_init, gae_sgns_walk_order, gae_sgns_accumulate,
gae_sgns_update; ops.random_walks, ops.sgns_noise_table, ops.sgns_train, ops.deepwalk), written from the K37 / K38 comment of
include/gae_hip_experimental.h: integer walks from Philox words, the noise table from the same numpy calls, negatives by
bisection of a 64-bit target, every product element one fp32 fma chain from +0 (mlp_ref.fma32), the fp64 sigma of K30
(boost_ref.sigma), int64 fixed-point accumulators that wrap, and the Adagrad sequence as single fp32 operations.  The device
must return the same bits.  Shared by tests/test_deepwalk_cpu.py and tests/test_gpu_deepwalk.py."""
import collections

import numpy as np

from boost_ref import sigma
from mlp_ref import _draw, f32, fma32, perm, philox

WALK_DRAW, NEG_DRAW, INIT_DRAW = 0x3700000000, 0x3800000000, 0x3900000000
NOISE_BITS, SCALE_BITS = 20, 32
ERR_RANGE, ERR_NONFINITE = 8, 64

State = collections.namedtuple("State", ["W", "C", "HW", "HC", "AW", "AC", "flags", "n_batches"])


def csr(n, src, dst):
    """(indptr int64 [n + 1], indices int64 [nnz]) as graph.csr() stores it: row = destination, columns = its sources
    ascending, duplicates kept"""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    order = np.lexsort((src, dst))
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(dst, minlength=n), out=indptr[1:])
    return indptr, src[order]


def random_walks(indptr, indices, starts=None, walks_per_start=10, length=40, seed=0):
    """int32 [m r, L]: walk w = rep m + s; step t takes word (t & 3) of philox(w, WALK_DRAW + (t >> 2), seed)"""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    n = indptr.shape[0] - 1
    starts = np.arange(n, dtype=np.int64) if starts is None else np.asarray(starts, np.int64)
    m = starts.shape[0]
    w = np.arange(m * walks_per_start, dtype=np.uint64)
    walks = np.full((w.shape[0], length), -1, np.int64)
    v = starts[(w % np.uint64(max(m, 1))).astype(np.int64)] if m else starts
    walks[:, 0] = v
    for t in range(1, length):
        word = philox(w, WALK_DRAW + (t >> 2), seed)[t & 3]
        safe = np.where(v >= 0, v, 0)
        deg = np.where(v >= 0, indptr[safe + 1] - indptr[safe], 0)
        off = ((word * deg.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
        at = np.minimum(indptr[safe] + off, max(indices.shape[0] - 1, 0))
        v = np.where(deg > 0, indices[at] if indices.shape[0] else -1, -1)
        walks[:, t] = v
    return walks.astype(np.int32)


def counts_of(walks, n):
    flat = np.asarray(walks).reshape(-1)
    return np.bincount(flat[flat >= 0], minlength=n).astype(np.int64)


def noise_table(walks, n, power=0.75):
    """int64 cum [n + 1]: cum[i + 1] = cum[i] + rint(2^20 count_i^power) where count_i > 0, + 0 elsewhere"""
    c = counts_of(walks, n).astype(np.float64)
    w = np.zeros(n, np.int64)
    seen = c > 0
    w[seen] = np.rint(np.float64(2.0) ** NOISE_BITS * np.power(c[seen], np.float64(power))).astype(np.int64)
    cum = np.zeros(n + 1, np.int64)
    np.cumsum(w, out=cum[1:])
    return cum


def init_table(n, dim, seed):
    return _draw(n * dim, INIT_DRAW, seed, f32(0.5 / dim)).reshape(n, dim)


def negatives(cum, seed, epoch, wids, M):
    """int64 [B, M]: slot s of walk w takes the 64-bit word (words 2 (s & 1) + 1 and 2 (s & 1)) of
    philox((epoch << 32) | w, NEG_DRAW + (s >> 1), seed); the node is the largest i of [0, n) with cum[i] <= target"""
    n = cum.shape[0] - 1
    total = int(cum[n])
    ctr = (np.uint64(epoch) << np.uint64(32)) | np.asarray(wids, np.uint64)
    out = np.zeros((ctr.shape[0], M), np.int64)
    for s in range(M):
        c = philox(ctr, NEG_DRAW + (s >> 1), seed)
        u = (c[2 * (s & 1) + 1] << np.uint64(32)) | c[2 * (s & 1)]
        target = np.asarray([(int(x) * total) >> 64 for x in u], np.int64)     # the high 64 bits of the 128-bit product
        out[:, s] = np.searchsorted(cum[:n], target, side="right") - 1
    return out


def chains(A, B):
    """fp32 [..., m, n]: element (i, j) is the chain c <- fma(A[..., i, k], B[..., k, j], c) from +0 over k ascending"""
    A, B = np.asarray(A, f32), np.asarray(B, f32)
    acc = np.zeros(A.shape[:-1] + (B.shape[-1],), f32)
    for k in range(A.shape[-1]):
        acc = fma32(A[..., :, k:k + 1], B[..., k:k + 1, :], acc)
    return acc


def batch_grads(ids, neg, W, C, window, K):
    """(dW [B, L, d], dC [B, L + M, d], valid [B, L]) of the walks ids int64 [B, L] with the negatives neg int64 [B, M]"""
    Bn, L = ids.shape
    M = neg.shape[1]
    valid = ids >= 0
    Ww = np.where(valid[..., None], W[np.where(valid, ids, 0)], f32(0.0)).astype(f32)
    Cw = np.where(valid[..., None], C[np.where(valid, ids, 0)], f32(0.0)).astype(f32)
    Cc = np.concatenate([Cw, C[neg]], axis=1)                                  # [B, L + M, d]
    SN = chains(Ww, np.swapaxes(Cc, 1, 2))                                     # [B, L, L + M]
    p = np.arange(L)
    dist = np.abs(p[:, None] - p[None, :])
    pos = (dist > 0) & (dist <= window) & valid[:, :, None] & valid[:, None, :]
    c = pos.sum(2)
    coef = (K * c).astype(f32) / f32(M)
    Gp = np.where(pos, sigma(-SN[:, :, :L].astype(np.float64)).astype(f32), f32(0.0)).astype(f32)
    Gn = -(coef[:, :, None] * sigma(SN[:, :, L:].astype(np.float64)).astype(f32))
    own = (neg[:, None, :] == ids[:, :, None]) | ~valid[:, :, None]
    Gn = np.where(own, f32(0.0), Gn).astype(f32)
    G = np.concatenate([Gp, Gn], axis=2)
    return chains(G, Cc), chains(np.swapaxes(G, 1, 2), Ww), valid


def scatter(acc, nodes, X):
    """adds llrint(x 2^32) of the rows X [r, d] to acc[nodes]; True when an element is outside the frame (not added)"""
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.abs(X) < f32(2.0 ** 20)                                        # (False for a NaN)
        q = np.where(ok, np.rint(np.where(ok, X, f32(0.0)).astype(np.float64) * 2.0 ** SCALE_BITS), 0.0).astype(np.int64)
    np.add.at(acc, nodes, q)                                                   # int64: wraps
    return bool((~ok).any())


def update(X, H, A, lr, eps):
    """Adagrad on the elements with a non-zero accumulator, in place; True when a new value is not finite"""
    m = A != 0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g = (A[m].astype(np.float64) * 2.0 ** -SCALE_BITS).astype(f32)
        h = fma32(g, g, H[m])
        s = np.sqrt(h) + f32(eps)
        q = g / s
        x = fma32(f32(lr), q, X[m])
    H[m], X[m], A[m] = h, x, 0
    return not (np.isfinite(x).all() and np.isfinite(h).all())


def train(walks, cum, W, C, HW, HC, *, window=5, negatives_per_pair=5, shared_negatives=16, epochs=3, batch_walks=256, lr=0.05,
          eps=1e-8, seed=0, first_epoch=0):
    """the State after the epochs; the inputs are not changed"""
    walks = np.asarray(walks, np.int64)
    W, C, HW, HC = (np.array(t, f32) for t in (W, C, HW, HC))
    AW, AC = np.zeros(W.shape, np.int64), np.zeros(W.shape, np.int64)
    n_walks = walks.shape[0]
    flags = n_batches = 0
    for epoch in range(first_epoch, first_epoch + epochs):
        order = perm(n_walks, seed, epoch)
        for first in range(0, n_walks, batch_walks):
            wids = order[first:first + batch_walks]
            ids = walks[wids]
            neg = negatives(cum, seed, epoch, wids, shared_negatives)
            dW, dC, valid = batch_grads(ids, neg, W, C, window, negatives_per_pair)
            L = ids.shape[1]
            bad = scatter(AW, ids[valid], dW[valid])
            bad = scatter(AC, ids[valid], dC[:, :L][valid]) or bad
            bad = scatter(AC, neg.reshape(-1), dC[:, L:].reshape(-1, W.shape[1])) or bad
            flags |= ERR_RANGE if bad else 0
            bad = update(W, HW, AW, lr, eps)
            bad = update(C, HC, AC, lr, eps) or bad
            flags |= ERR_NONFINITE if bad else 0
            n_batches += 1
    return State(W, C, HW, HC, AW, AC, flags, n_batches)


def deepwalk(indptr, indices, dim, *, walks_per_node=10, walk_length=40, window=5, negatives_per_pair=5, shared_negatives=16,
             epochs=3, batch_walks=256, lr=0.05, eps=1e-8, noise_power=0.75, seed=0, walks=None):
    """(State, walks, cum) of ops.deepwalk with the same arguments"""
    n = np.asarray(indptr).shape[0] - 1
    if walks is None:
        walks = random_walks(indptr, indices, None, walks_per_node, walk_length, seed)
    cum = noise_table(walks, n, noise_power)
    zeros = np.zeros((n, dim), f32)
    st = train(walks, cum, init_table(n, dim, seed), zeros, zeros, zeros, window=window,
               negatives_per_pair=negatives_per_pair, shared_negatives=shared_negatives, epochs=epochs, batch_walks=batch_walks,
               lr=lr, eps=eps, seed=seed)
    return st, walks, cum


def walk_graph():
    """70 nodes: a random symmetric part on 0..66 with duplicate edges and self-loops, node 67 isolated, node 68 a directed
    sink row (edges lead away from it in csr terms: it is a source of others' rows, its own row is empty), node 69 a hub row
    of 300 entries (duplicates included)"""
    rng = np.random.default_rng(7)
    a, b = rng.integers(0, 67, 160), rng.integers(0, 67, 160)
    a, b = np.concatenate([a, a[:10], [3, 8]]), np.concatenate([b, b[:10], [3, 8]])          # duplicates, two self-loops
    src, dst = np.concatenate([a, b]), np.concatenate([b, a])
    src, dst = np.concatenate([src, [68, 68, 68]]), np.concatenate([dst, [1, 2, 5]])         # 68 is listed, lists nothing
    hub = rng.integers(0, 67, 300)
    src, dst = np.concatenate([src, hub, [69, 69]]), np.concatenate([dst, np.full(300, 69), [4, 6]])
    return 70, src.astype(np.int64), dst.astype(np.int64)


def two_blocks(seed=0, size=32, p_in=0.3, p_out=0.02):
    """(n, src, dst, block): the two-block graph of the learning condition, both directions listed"""
    rng = np.random.default_rng(seed)
    n = 2 * size
    block = np.arange(n) // size
    i, j = np.triu_indices(n, 1)
    keep = rng.random(i.shape[0]) < np.where(block[i] == block[j], p_in, p_out)
    i, j = i[keep], j[keep]
    return n, np.concatenate([i, j]).astype(np.int64), np.concatenate([j, i]).astype(np.int64), block


def auc(scores, labels):
    """ROC-AUC by ranks, ties at their mean rank"""
    scores, labels = np.asarray(scores, np.float64), np.asarray(labels, bool)
    order = np.argsort(scores, kind="stable")
    ranks = np.empty(scores.shape[0], np.float64)
    sorted_scores = scores[order]
    uniq, start, cnt = np.unique(sorted_scores, return_index=True, return_counts=True)
    mean_rank = start + (cnt + 1) / 2.0
    ranks[order] = np.repeat(mean_rank, cnt)
    n_pos, n_neg = int(labels.sum()), int((~labels).sum())
    return (ranks[labels].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg)


def same_block_auc(W, block):
    """ROC-AUC of the cosine similarity over all node pairs against 'same block'"""
    Z = np.asarray(W, np.float64)
    Z = Z / np.maximum(np.linalg.norm(Z, axis=1, keepdims=True), 1e-30)
    i, j = np.triu_indices(Z.shape[0], 1)
    return auc((Z[i] * Z[j]).sum(1), block[i] == block[j])
