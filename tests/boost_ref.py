"""numpy restatement of K30 (gae_boost_fit / gae_boost_predict, ops.boost), written from the K30 comment of
include/gae_hip_experimental.h: the fixed-point frame, the restated sigma, the round prologue with its held-out loss in
the stated order, histogram growth with the second-order score as plain fp64 numpy operations, the tie rules, node
numbering, leaf weights, the CV curve and the selection rule, prediction.  Every accumulated quantity is an integer, so
the device must reproduce each tree node for node and each value bit for bit.  Shared by tests/test_boost_cpu.py and
tests/test_gpu_boost.py."""
import collections
import math

import numpy as np

from forest_ref import SPLIT_ROWS, feature_subset, make_codes, make_edges, philox  # noqa: F401  (philox: re-exported)

INV_LN2, LN2_HI, LN2_LO, CLAMP = 1.44269504088896338700e+00, 6.93147180369123816490e-01, 1.90821492927058770002e-10, 40.0
COEF = [1.0 / math.factorial(j) for j in range(13, -1, -1)]           # 1/13! .. 1/0!, correctly rounded quotients
FRAME = 2147483648.0
MAX_D, MAX_BINS, MAX_DEPTH, MAX_ROUNDS, MAX_MODELS = 256, 256, 8, 4096, 256

Boost = collections.namedtuple("Boost", [
    "feature", "threshold_bin", "threshold", "left", "count", "value", "gain", "n_nodes", "base_score", "edges", "n_edges",
    "lr", "lam", "best_round", "best_cfg", "cv_curve", "cv_rmse", "cv_r2", "cv_logloss", "cv_accuracy", "importances",
    "info", "train_score", "objective", "n_used", "rows", "fold", "loss", "correct", "exponent"])


def exp_neg(a):
    """exp(-a) for 0 <= a <= 40 as the header states it: two-part ln 2 reduction, degree-13 Horner, exact 2^k scaling"""
    a = np.asarray(a, np.float64)
    t = -a
    k = np.rint(t * INV_LN2)
    r = (t - k * LN2_HI) - k * LN2_LO
    p = np.full_like(r, COEF[0])
    for c in COEF[1:]:
        p = p * r + c
    return p * np.ldexp(1.0, k.astype(np.int64))


def clamp_abs(F):
    a = np.abs(np.asarray(F, np.float64))
    return np.where(a < CLAMP, a, CLAMP)


def sigma(F):
    F = np.asarray(F, np.float64)
    e = exp_neg(clamp_abs(F))
    q = e / (1.0 + e)
    return np.where(F >= 0.0, 1.0 - q, q)


def frame(ys, objective):
    """(base_score, exponent) of the listed targets"""
    if objective == "logistic":
        return 0.0, 30
    base = float(np.float32(math.fsum(ys.astype(np.float64).tolist()) / len(ys)))
    spread = float(np.abs(ys.astype(np.float64) - base).max())
    return base, (0 if spread == 0.0 else 29 - math.frexp(spread)[1])


def wave_tree(v):
    """lane 0 of the shuffle-down tree 32, 16, .., 1 over 64 lanes; v [..., 64]"""
    for off in (32, 16, 8, 4, 2, 1):
        v = v[..., :off] + v[..., off:2 * off]
    return v[..., 0]


def chunk_sums(v):
    """per chunk of 256 rows: the four waves' trees, then ((w0 + w1) + w2) + w3"""
    n = len(v)
    parts = -(-n // 256)
    pad = np.zeros(parts * 256)
    pad[:n] = v
    w = wave_tree(pad.reshape(parts, 4, 64))
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def fold_partials(p):
    """the order of csrc/common.h's sum_partials"""
    n = len(p)
    if n <= 32:
        g = np.float64(0.0)
        for v in p:
            g = g + v
        return g
    lanes = np.zeros(64)
    for q in range(n):
        lanes[q % 64] = lanes[q % 64] + p[q]                           # (q ascending: each lane adds its own in order)
    return wave_tree(lanes)


def leaf_weight(G, H, g_step, h_step, lr, lam):
    g, den = np.float64(G) * g_step, np.float64(H) * h_step + lam
    return -(lr * (g / den)) if den > 0.0 else np.float64(0.0)


def parent_score(G, H, g_step, h_step, lam):
    g, den = np.float64(G) * g_step, np.float64(H) * h_step + lam
    return (g * g) / den if den > 0.0 else np.float64(0.0)


def candidate_scores(GL, HL, G, H, nl, n, g_step, h_step, lam, msl, mcw):
    """(score, ok) of every cell: GL, HL int64 prefix sums [...], nl counts [...]"""
    gl, gr = GL.astype(np.float64) * g_step, (G - GL).astype(np.float64) * g_step
    hl, hr = HL.astype(np.float64) * h_step, (H - HL).astype(np.float64) * h_step
    dl, dr = hl + lam, hr + lam
    ok = (nl >= msl) & (n - nl >= msl) & (hl >= mcw) & (hr >= mcw) & (dl > 0.0) & (dr > 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = (gl * gl) / dl + (gr * gr) / dr
    return sc, ok


def grow_tree(draw, samples, codes, gq, hq, n_edges, edges, bins, g_step, h_step, lr, lam, max_depth, m_feat, msl, mcw,
              min_gain, seed, M):
    """one tree on the listed rows `samples` (gq, hq indexed by listed row); draw = (round << 8) | fold slot"""
    d = codes.shape[1]
    feature = np.full(M, -1, np.int32); tbin = np.full(M, -1, np.int32); left = np.full(M, -1, np.int32)
    count = np.zeros(M, np.int32); threshold = np.zeros(M, np.float32)
    value = np.zeros(M, np.float64); gain = np.zeros(M, np.float64)
    sums = {0: (int(gq[samples].sum()), int(hq[samples].sum()))}
    count[0] = len(samples)
    value[0] = leaf_weight(*sums[0], g_step, h_step, lr, lam)
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
            GL = np.zeros(d * bins, np.int64); HL = np.zeros(d * bins, np.int64)
            np.add.at(GL, flat, np.repeat(gq[s], d))
            np.add.at(HL, flat, np.repeat(hq[s], d))
            GL, HL = GL.reshape(d, bins).cumsum(1), HL.reshape(d, bins).cumsum(1)
            G, H = sums[node]
            sc, ok = candidate_scores(GL, HL, G, H, cnt, n, g_step, h_step, lam, msl, mcw)
            ok &= valid_b & feature_subset(draw, node, d, m_feat, seed)[:, None]
            if not ok.any():
                continue
            sc = np.where(ok, sc, -np.inf)
            at = int(np.argmax(sc))                                    # the first maximum: the lower f, then the lower b
            f, b = divmod(at, bins)
            best, parent = sc[f, b], parent_score(G, H, g_step, h_step, lam)
            if not best > parent + min_gain:
                continue
            L = base + 2 * k
            k += 1
            feature[node], tbin[node], left[node] = f, b, L
            threshold[node], gain[node] = edges[f, b], best - parent
            go = codes[s, f] <= b
            gl, hl = int(GL[f, b]), int(HL[f, b])
            for c, part, Sc in ((L, s[go], (gl, hl)), (L + 1, s[~go], (G - gl, H - hl))):
                count[c] = len(part)
                sums[c] = Sc
                value[c] = leaf_weight(*Sc, g_step, h_step, lr, lam)
                nxt.append((c, part))
            assert count[L] == cnt[f, b]
        n_nodes = base + 2 * k
        level = nxt
        if not level:
            break
    return feature, tbin, threshold, left, count, value, gain, n_nodes


def leaf_values(tree, codes):
    """fp64 [n]: the value of the leaf every row of `codes` reaches"""
    feature, tbin, _, left, _, value = tree[:6]
    node = np.zeros(len(codes), np.int64)
    for _ in range(MAX_DEPTH):
        f = feature[node]
        inner = f >= 0
        go = codes[np.arange(len(codes)), np.where(inner, f, 0)] <= tbin[node]
        node = np.where(inner, left[node] + np.where(go, 0, 1), node)
    return value[node]


def default_fold(n, F, seed):
    import torch
    if F <= 1:
        return np.zeros(n, np.int64)
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    perm = torch.randperm(n, generator=g)
    fold = torch.empty(n, dtype=torch.int64)
    fold[perm] = torch.arange(n) % F
    return fold.numpy()


def choose(cv_curve, ok):
    """(cfg, round index): the smallest pooled held-out loss among the eligible configurations, ties to the lower cfg, then
    the lower round; (-1, -1): none"""
    best = (-1, -1)
    for c in range(cv_curve.shape[0]):
        if not ok[c]:
            continue
        for r in range(cv_curve.shape[1]):
            v = cv_curve[c, r]
            if not math.isnan(v) and (best[0] < 0 or v < cv_curve[best]):
                best = (c, r)
    return best


def importances(feature, gain, d):
    on = feature >= 0
    f, w = feature[on], gain[on]
    sums = [math.fsum(w[f == q].tolist()) for q in range(d)]
    total = math.fsum(sums)
    return np.array([s / total if total > 0.0 else 0.0 for s in sums])


def boost(X, y, objective="squared", n_rounds=100, *, max_depth=4, learning_rates=(0.1,), lambdas=(1.0,),
          min_child_weight=1.0, min_samples_leaf=1, min_gain=0.0, max_features=1.0, max_bins=64, folds=5, fold=None,
          rows=None, seed=0):
    """ops.boost on numpy arrays"""
    X = np.asarray(X, np.float32)
    y = np.asarray(y)
    n = len(X)
    keep = np.zeros(n, bool)
    if rows is None:
        keep[:] = True
    else:
        rows = np.asarray(rows)
        keep[np.nonzero(rows)[0] if rows.dtype == bool else rows] = True
    fold = default_fold(n, folds, seed) if fold is None else np.asarray(fold).astype(np.int64)
    keep &= fold >= 0
    if objective == "logistic":
        keep &= y >= 0
    listed = np.nonzero(keep)[0]
    Xs, ys, fo = X[listed], y[listed].astype(np.float32), fold[listed]
    n_used, d = Xs.shape
    F = folds if folds > 1 else 0
    cfgs = [(float(lr), float(lam)) for lr in learning_rates for lam in lambdas]
    m_feat = max_features if isinstance(max_features, int) else max(1, int(max_features * d))
    M = 2 ** (max_depth + 1) - 1
    R = n_rounds
    edges, n_edges = make_edges(Xs, max_bins)
    codes = make_codes(Xs, edges, n_edges)
    base, e = frame(ys, objective)
    logistic = objective == "logistic"
    g_up = math.ldexp(1.0, e); g_step = math.ldexp(1.0, -e)
    h_up, h_step = (g_up, g_step) if logistic else (1.0, 1.0)
    yd = ys.astype(np.float64)
    Mo = (F + 1) * len(cfgs)
    loss = np.zeros((Mo, R + 1)); correct = np.zeros((Mo, R + 1), np.int64); bad = np.zeros(Mo, bool)
    score = np.zeros((Mo, n_used))
    tables = [[None] * R for _ in cfgs]
    for m in range(Mo):
        c, k = divmod(m, F + 1)
        lr, lam = cfgs[c]
        held = (fo == k) if k < F else np.zeros(n_used, bool)
        train = np.nonzero(~held)[0]
        Fs = np.full(n_used, base)
        tree = None
        for r in range(R + 1):
            if r > 0:
                Fs = Fs + leaf_values(tree, codes)
            if not np.isfinite(Fs).all():
                bad[m] = True
            if logistic:
                ex = exp_neg(clamp_abs(Fs))
                q = ex / (1.0 + ex)
                p = np.where(Fs >= 0.0, 1.0 - q, q)
                g, h = p - yd, p * (1.0 - p)
                agree = (Fs >= 0.0) == (ys > 0.5)
                ls = np.log1p(ex) + np.where(agree, 0.0, np.abs(Fs))
                correct[m, r] = int((agree & held).sum())
            else:
                g = Fs - yd
                ls = g * g
            loss[m, r] = fold_partials(chunk_sums(np.where(held, ls, 0.0)))
            if r == R:
                break
            vg = g * g_up
            inside = np.abs(vg) <= FRAME
            gq = np.where(inside, np.rint(np.where(inside, vg, 0.0)), 0.0).astype(np.int64)
            if logistic:
                vh = h * h_up
                hq = np.rint(vh).astype(np.int64)
            else:
                hq = np.ones(n_used, np.int64)
            if not inside[train].all():
                bad[m] = True
            tree = grow_tree((r << 8) | k, train, codes, gq, hq, n_edges, edges, max_bins, g_step, h_step, lr, lam, max_depth,
                             m_feat, min_samples_leaf, min_child_weight, min_gain, seed, M)
            if k == F:
                tables[c][r] = tree
        score[m] = Fs
    info = np.array([int(bad[c * (F + 1):(c + 1) * (F + 1)].any()) for c in range(len(cfgs))], np.int32)
    nan = float("nan")
    cv_rmse = cv_r2 = cv_logloss = cv_acc = nan
    if F:
        pooled = np.zeros((len(cfgs), R))
        for c in range(len(cfgs)):
            acc = loss[c * (F + 1), 1:].copy()
            for k in range(1, F):
                acc = acc + loss[c * (F + 1) + k, 1:]
            pooled[c] = acc
        cv_curve = pooled / np.float64(n_used)
        bc, br = choose(cv_curve, info == 0)
        if bc < 0:
            raise RuntimeError("no configuration stayed finite")
        if logistic:
            cv_logloss = cv_curve[bc, br]
            cv_acc = sum(int(correct[bc * (F + 1) + k, br + 1]) for k in range(F)) / np.float64(n_used)
        else:
            mean = math.fsum(yd.tolist()) / n_used
            sst = math.fsum(((yd - mean) * (yd - mean)).tolist())
            cv_rmse = math.sqrt(cv_curve[bc, br])
            cv_r2 = 1.0 - pooled[bc, br] / sst if sst > 0.0 else nan
    else:
        cv_curve = np.full((len(cfgs), R), nan)
        bc, br = 0, R - 1
        if info[0]:
            raise RuntimeError("no configuration stayed finite")
    cols = [np.stack(col) for col in zip(*tables[bc])]
    best_round = br + 1
    return Boost(*cols[:7], np.array(cols[7], np.int32), base, edges, n_edges, cfgs[bc][0], cfgs[bc][1], best_round, bc,
                 cv_curve, cv_rmse, cv_r2, cv_logloss, cv_acc,
                 importances(cols[0][:best_round], cols[6][:best_round], d), info, score[bc * (F + 1) + F], objective, n_used,
                 listed, fo, loss, correct, e)


def predict(model, X, n_rounds=None):
    """fp64 [m]: base_score + the leaves' values in ascending round order on the raw fp32 values; NaN for a row with a
    non-finite feature"""
    X = np.asarray(X, np.float32)
    R = model.best_round if n_rounds is None else n_rounds
    out = np.full(len(X), np.nan)
    for i in range(len(X)):
        if not np.isfinite(X[i]).all():
            continue
        acc = np.float64(model.base_score)
        for r in range(R):
            node = 0
            while model.feature[r, node] >= 0:
                node = model.left[r, node] + (0 if X[i, model.feature[r, node]] <= model.threshold[r, node] else 1)
            acc = acc + model.value[r, node]
        out[i] = acc
    return out
