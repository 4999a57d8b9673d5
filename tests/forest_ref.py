"""numpy restatement of K26 (gae_forest_bin / gae_forest_fit / gae_forest_predict, ops.forest), written from the K26
comment of include/gae_hip_experimental.h: edges, codes, fixed-point targets, the Philox bootstrap and feature subsets,
level-wise growth with the stated score order as plain fp64 numpy operations, node numbering, values, prediction,
out-of-bag scores and importances.  Every accumulated quantity is an integer, so the device must reproduce each tree
node for node and each value bit for bit.  Shared by tests/test_forest_cpu.py and tests/test_gpu_forest.py."""
import collections
import math

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
KEY_XOR = 0xA0761D6478BD642F
SPLIT_ROWS = 8192

Forest = collections.namedtuple("Forest", [
    "feature", "threshold_bin", "threshold", "left", "count", "value", "gain", "n_nodes", "edges", "n_edges",
    "oob_prediction", "oob_rmse", "oob_r2", "importances", "n_used", "pivot", "exponent", "samples", "codes", "yq"])


def philox(ctr, draw, key):
    """philox4x32_10 of csrc/common.h over an array of counters: uint64 [4, len] holding the four 32-bit words"""
    ctr = np.asarray(ctr, np.uint64).reshape(-1)
    c = [ctr & M32, ctr >> np.uint64(32), np.full_like(ctr, draw & 0xFFFFFFFF), np.full_like(ctr, (draw >> 32) & 0xFFFFFFFF)]
    k0, k1 = key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)) & M32, p1 & M32,
             ((p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)) & M32, p0 & M32]
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c)


def bootstrap_rows(tree, n_boot, n_used, seed):
    """the listed rows tree `tree` trains on: sample j is (w n_used) >> 32, w = word j & 3 of block j >> 2"""
    j = np.arange(n_boot, dtype=np.uint64)
    words = philox(j >> np.uint64(2), tree, seed ^ KEY_XOR)
    w = words[(j & np.uint64(3)).astype(np.int64), np.arange(n_boot)]
    return ((w * np.uint64(n_used)) >> np.uint64(32)).astype(np.int64)


def feature_subset(tree, node, d, m, seed):
    """bool [d]: the m features with the smallest (r_f, f)"""
    if m >= d:
        return np.ones(d, bool)
    f = np.arange(d, dtype=np.uint64)
    r = philox((np.uint64(node) << np.uint64(8)) | f, (1 << 32) + tree, seed ^ KEY_XOR)[0]
    order = np.lexsort((np.arange(d), r))
    sel = np.zeros(d, bool)
    sel[order[:m]] = True
    return sel


def make_edges(Xs, max_bins):
    """(edges fp32 [d, max_bins - 1] padded with +inf, n_edges int32 [d])"""
    n, d = Xs.shape
    E = max_bins - 1
    edges = np.full((d, E), np.inf, np.float32)
    n_edges = np.zeros(d, np.int32)
    for f in range(d):
        v = np.sort(Xs[:, f])
        u = np.unique(v)
        if len(u) <= max_bins:
            a, b = u[:-1], u[1:]
            mid = ((a.astype(np.float64) + b.astype(np.float64)) / 2).astype(np.float32)
            e = np.where(mid >= b, a, mid)
        else:
            q = v[(np.arange(1, max_bins, dtype=np.int64) * n) // max_bins]
            e = q[np.concatenate([[True], q[1:] != q[:-1]])]
        edges[f, :len(e)] = e
        n_edges[f] = len(e)
    return edges + np.float32(0), n_edges                              # an edge of -0 is stored as +0


def make_codes(Xs, edges, n_edges):
    """uint8 [n, d]: code(x) = #{e in edges[f] : e < x}"""
    return np.stack([np.searchsorted(edges[f, :n_edges[f]], Xs[:, f], side="left") for f in range(Xs.shape[1])],
                    1).astype(np.uint8)


def target_frame(Ys):
    """(pivot fp32 [t], exponent [t]): the fp64 mean rounded to fp32, e = 30 - E of frexp(max |y - c|)"""
    n, t = Ys.shape
    pivot = np.array([math.fsum(Ys[:, j].astype(np.float64).tolist()) / n for j in range(t)]).astype(np.float32)
    spread = np.abs(Ys.astype(np.float64) - pivot.astype(np.float64)).max(0)
    return pivot, [0 if s == 0.0 else 30 - math.frexp(float(s))[1] for s in spread]


def quantise(Ys, pivot, exponent):
    up = np.array([math.ldexp(1.0, e) for e in exponent])
    return np.rint((Ys.astype(np.float64) - pivot.astype(np.float64)) * up).astype(np.int64)


def score_of(SL, SR, nl, nr, scale):
    """the candidate score in the header's order: convert, square, divide, add the sides, scale, add over j ascending.
    SL, SR int64 [..., t]; nl, nr int arrays [...]"""
    score = np.zeros(np.shape(nl), np.float64)
    fl, fr = np.asarray(nl, np.float64), np.asarray(nr, np.float64)
    for j in range(len(scale)):
        dl, dr = SL[..., j].astype(np.float64), SR[..., j].astype(np.float64)
        term = (dl * dl / fl + dr * dr / fr) * scale[j]
        score = score + term
    return score


def parent_score(S, n, scale):
    p = np.float64(0.0)
    for j in range(len(scale)):
        ds = np.float64(S[j])
        p = p + (ds * ds / np.float64(n)) * scale[j]
    return p


def node_value(S, n, pivot, exponent):
    return np.array([np.float64(pivot[j]) + (np.float64(S[j]) / np.float64(n)) * math.ldexp(1.0, -exponent[j])
                     for j in range(len(exponent))])


def grow_tree(tree, samples, codes, yq, n_edges, edges, bins, pivot, exponent, max_depth, m_feat, msl, seed, M):
    d, t = codes.shape[1], yq.shape[1]
    scale = [math.ldexp(1.0, -2 * e) for e in exponent]
    feature = np.full(M, -1, np.int32); tbin = np.full(M, -1, np.int32); left = np.full(M, -1, np.int32)
    count = np.zeros(M, np.int32); threshold = np.zeros(M, np.float32)
    value = np.zeros((M, t), np.float64); gain = np.zeros(M, np.float64)
    sums = {0: yq[samples].sum(0)}
    count[0] = len(samples)
    value[0] = node_value(sums[0], len(samples), pivot, exponent)
    n_nodes = 1
    level = [(0, samples)]
    valid_b = np.arange(bins)[None, :] < n_edges[:, None]              # [d, bins]
    for depth in range(max_depth):
        base, k, nxt = n_nodes, 0, []
        for node, s in level:                                          # ascending node id
            n = len(s)
            if n < 2 * msl:
                continue
            flat = (np.arange(d)[None, :] * bins + codes[s]).reshape(-1)
            cnt = np.bincount(flat, minlength=d * bins).reshape(d, bins).cumsum(1)
            SL = np.zeros((d * bins, t), np.int64)
            for j in range(t):
                np.add.at(SL[:, j], flat, np.repeat(yq[s, j], d))
            SL = SL.reshape(d, bins, t).cumsum(1)
            S = sums[node]
            nl, nr = cnt, n - cnt
            ok = valid_b & feature_subset(tree, node, d, m_feat, seed)[:, None] & (nl >= msl) & (nr >= msl)
            if not ok.any():
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                sc = score_of(SL, S[None, None, :] - SL, nl, nr, scale)
            sc = np.where(ok, sc, -np.inf)
            at = int(np.argmax(sc))                                    # the first maximum: the lower f, then the lower b
            f, b = divmod(at, bins)
            best, parent = sc[f, b], parent_score(S, n, scale)
            if not best > parent:
                continue
            L = base + 2 * k
            k += 1
            feature[node], tbin[node], left[node] = f, b, L
            threshold[node], gain[node] = edges[f, b], best - parent
            go = codes[s, f] <= b
            for c, part, Sc in ((L, s[go], SL[f, b]), (L + 1, s[~go], S - SL[f, b])):
                count[c] = len(part)
                sums[c] = Sc
                value[c] = node_value(Sc, len(part), pivot, exponent)
                nxt.append((c, part))
            assert count[L] == nl[f, b]
        n_nodes = base + 2 * k
        level = nxt
        if not level:
            break
    return feature, tbin, threshold, left, count, value, gain, n_nodes


def predict(model, X, skip=None):
    """fp64 [m, t]: every row walks every tree on the raw fp32 values; skip bool [T, m] omits trees; NaN for a row with a
    non-finite feature or without a tree"""
    X = np.asarray(X, np.float32)
    m, T, t = X.shape[0], model.feature.shape[0], model.value.shape[2]
    out = np.full((m, t), np.nan)
    for i in range(m):
        if not np.isfinite(X[i]).all():
            continue
        acc, used = np.zeros(t), 0
        for tr in range(T):
            if skip is not None and skip[tr, i]:
                continue
            node = 0
            while model.feature[tr, node] >= 0:
                node = model.left[tr, node] + (0 if X[i, model.feature[tr, node]] <= model.threshold[tr, node] else 1)
            acc = acc + model.value[tr, node]
            used += 1
        if used:
            out[i] = acc / np.float64(used)
    return out


def leaf_of(model, tree, x):
    node = 0
    while model.feature[tree, node] >= 0:
        node = model.left[tree, node] + (0 if x[model.feature[tree, node]] <= model.threshold[tree, node] else 1)
    return node


def fsum_scores(pred, y):
    t = y.shape[1]
    rmse, r2 = np.full(t, np.nan), np.full(t, np.nan)
    for j in range(t):
        keep = ~np.isnan(pred[:, j])
        p, v = pred[keep, j], y[keep, j].astype(np.float64)
        k = len(p)
        if k == 0:
            continue
        r = p - v
        sse = math.fsum((r * r).tolist())
        mean = math.fsum(v.tolist()) / k
        c = v - mean
        sst = math.fsum((c * c).tolist())
        rmse[j] = math.sqrt(sse / k)
        r2[j] = 1.0 - sse / sst if sst > 0.0 else np.nan
    return rmse, r2


def importances(feature, count, gain, d):
    on = feature >= 0
    f, w = feature[on], gain[on] * count[on].astype(np.float64)
    sums = [math.fsum(w[f == q].tolist()) for q in range(d)]
    total = math.fsum(sums)
    return np.array([s / total if total > 0.0 else 0.0 for s in sums])


def forest(X, y, n_trees=100, *, max_depth=12, max_features=1.0, min_samples_leaf=1, max_bins=64, bootstrap=True,
           max_samples=None, rows=None, seed=0):
    """ops.forest on numpy arrays"""
    X = np.asarray(X, np.float32)
    y = np.asarray(y, np.float32)
    Y = y.reshape(len(y), -1)
    if rows is None:
        rows = np.arange(len(X))
    rows = np.asarray(rows)
    if rows.dtype == bool:
        rows = np.nonzero(rows)[0]
    Xs, Ys = X[rows], Y[rows]
    n_used, d = Xs.shape
    t = Ys.shape[1]
    m_feat = max_features if isinstance(max_features, int) else max(1, int(max_features * d))
    n_boot = n_used if max_samples is None else \
        (max_samples if isinstance(max_samples, int) else max(1, int(max_samples * n_used)))
    M = min(2 ** (max_depth + 1) - 1, 2 * n_boot - 1)
    edges, n_edges = make_edges(Xs, max_bins)
    codes = make_codes(Xs, edges, n_edges)
    pivot, exponent = target_frame(Ys)
    yq = quantise(Ys, pivot, exponent)
    trees, samples = [], []
    for tr in range(n_trees):
        s = bootstrap_rows(tr, n_boot, n_used, seed) if bootstrap else np.arange(n_used)
        samples.append(s)
        trees.append(grow_tree(tr, s, codes, yq, n_edges, edges, max_bins, pivot, exponent, max_depth, m_feat,
                               min_samples_leaf, seed, M))
    cols = [np.stack(c) for c in zip(*trees)]
    model = Forest(*cols[:7], np.array(cols[7], np.int32), edges, n_edges, None, None, None, None, n_used, pivot, exponent,
                   samples, codes, yq)
    if bootstrap:
        inbag = np.zeros((n_trees, n_used), bool)
        for tr, s in enumerate(samples):
            inbag[tr, s] = True
        oob = predict(model, Xs, skip=inbag)
        rmse, r2 = fsum_scores(oob, Ys)
    else:
        oob = np.full((n_used, t), np.nan)
        rmse = r2 = np.full(t, np.nan)
    return model._replace(oob_prediction=oob, oob_rmse=rmse, oob_r2=r2,
                          importances=importances(model.feature, model.count, model.gain, d))
