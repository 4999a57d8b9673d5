"""Link-prediction evaluation the reference only alludes to (``# TODO: train test
split`` at gae_dgl/train_transductive.py:35, Kipf & Welling's AUC / AP protocol):
edge split into train / validation / test positives with sampled negatives,
ROC-AUC and average precision of ``sigmoid(z_i . z_j)``.

Evaluation utilities, not part of the HIP hot path: index bookkeeping and
rank statistics through torch ops on whatever device the tensors live on."""
import numpy as np
import torch


def split_edges(src, dst, n, val_frac=0.05, test_frac=0.10, seed=0):
    """Undirected split (both directions of a pair stay together).  Returns
    ``train (src, dst)`` with both directions, and ``val`` / ``test`` dicts with
    ``pos`` and ``neg`` int64 arrays of shape [2, k] (one direction per pair;
    negatives are sampled non-edges, no self pairs)."""
    src = np.asarray(src, dtype=np.int64); dst = np.asarray(dst, dtype=np.int64)
    rng = np.random.default_rng(seed)
    lo, hi = np.minimum(src, dst), np.maximum(src, dst)
    keep = lo != hi
    pairs = np.unique(np.stack([lo[keep], hi[keep]], 1), axis=0)
    perm = rng.permutation(len(pairs))
    n_val, n_test = int(len(pairs) * val_frac), int(len(pairs) * test_frac)
    val_p, test_p, train_p = pairs[perm[:n_val]], pairs[perm[n_val:n_val + n_test]], pairs[perm[n_val + n_test:]]
    edge_keys = set((pairs[:, 0] * n + pairs[:, 1]).tolist())

    def negatives(k):
        out = []
        while len(out) < k:
            a = rng.integers(0, n, 2 * (k - len(out)) + 8); b = rng.integers(0, n, a.size)
            for x, y in zip(np.minimum(a, b).tolist(), np.maximum(a, b).tolist()):
                if x != y and (x * n + y) not in edge_keys:
                    edge_keys.add(x * n + y)
                    out.append((x, y))
                    if len(out) == k:
                        break
        return np.asarray(out, dtype=np.int64).reshape(-1, 2).T

    train = (np.concatenate([train_p[:, 0], train_p[:, 1]]), np.concatenate([train_p[:, 1], train_p[:, 0]]))
    return train, {"pos": val_p.T.copy(), "neg": negatives(n_val)}, {"pos": test_p.T.copy(), "neg": negatives(n_test)}


def edge_scores(Z, pairs):
    """sigmoid(z_i . z_j) for pairs [2, k] (the decoder of gae.py:69-72 restricted to the listed pairs)"""
    pairs = torch.as_tensor(pairs, device=Z.device)
    return torch.sigmoid((Z[pairs[0]] * Z[pairs[1]]).sum(1))


def roc_auc(pos_scores, neg_scores):
    """area under the ROC curve = P(score_pos > score_neg) + 0.5 P(equal), via average ranks"""
    s = torch.cat([pos_scores, neg_scores]).double()
    n_pos, n_neg = pos_scores.numel(), neg_scores.numel()
    order = torch.argsort(s)
    sv = s[order]
    ranks = torch.arange(1, s.numel() + 1, device=s.device, dtype=torch.float64)
    # average ranks over ties
    uniq, inv, counts = torch.unique_consecutive(sv, return_inverse=True, return_counts=True)
    ends = torch.cumsum(counts, 0).double()
    avg = ends - (counts.double() - 1) / 2
    r = torch.empty_like(ranks)
    r[order] = avg[inv]
    return float((r[:n_pos].sum() - n_pos * (n_pos + 1) / 2) / (n_pos * n_neg))


def average_precision(pos_scores, neg_scores):
    """sum_k (R_k - R_{k-1}) P_k over distinct thresholds (sklearn's definition)"""
    s = torch.cat([pos_scores, neg_scores]).double()
    y = torch.cat([torch.ones_like(pos_scores), torch.zeros_like(neg_scores)]).double()
    order = torch.argsort(s, descending=True)
    s, y = s[order], y[order]
    tp = torch.cumsum(y, 0)
    k = torch.arange(1, s.numel() + 1, device=s.device, dtype=torch.float64)
    last = torch.ones_like(y, dtype=torch.bool)
    last[:-1] = s[1:] != s[:-1]                       # evaluate only at the end of each tie group
    prec, rec = (tp / k)[last], (tp / y.sum())[last]
    rec_prev = torch.cat([torch.zeros(1, device=s.device, dtype=torch.float64), rec[:-1]])
    return float(((rec - rec_prev) * prec).sum())


def evaluate(Z, split):
    p, q = edge_scores(Z, split["pos"]), edge_scores(Z, split["neg"])
    return {"auc": roc_auc(p, q), "ap": average_precision(p, q)}


def evaluate_scores(pos_scores, neg_scores):
    """{"auc", "ap"} of scores that are already per pair (a heuristic of ops.neighbour_scores, any monotone score): the
    ROC-AUC and AP ``evaluate`` reports for an embedding, ties at their average rank"""
    p, q = torch.as_tensor(pos_scores).reshape(-1), torch.as_tensor(neg_scores).reshape(-1)
    q = q.to(p.device)
    return {"auc": roc_auc(p, q), "ap": average_precision(p, q)}


def recall_at_k(index, pos_pairs):
    """fraction of the held-out positive pairs (i, j) (``pos_pairs`` [2, m]) found by a top-k list: j in row i of
    ``index`` [n, k] or i in row j (a link is undirected).  Duplicate pairs -- also (i, j) next to (j, i) -- count
    once; -1 entries (padding) match nothing.  An empty pair list gives NaN."""
    index = torch.as_tensor(index)
    pairs = torch.as_tensor(pos_pairs, device=index.device).long().reshape(2, -1)
    n = index.shape[0]
    a, b = torch.minimum(pairs[0], pairs[1]), torch.maximum(pairs[0], pairs[1])
    keys = torch.unique(a * n + b)
    if keys.numel() == 0:
        return float("nan")
    rows = torch.arange(n, device=index.device).unsqueeze(1).expand_as(index)
    ok = index >= 0
    i, j = rows[ok], index[ok].long()
    found = torch.unique(torch.minimum(i, j) * n + torch.maximum(i, j))
    return float(torch.isin(keys, found).double().mean())


def rank_metrics(greater, equal, candidates, ks=(1, 10, 50, 100)):
    """The filtered ranking protocol from the counts of ``GAE.rank_links`` / ``ops.decoder_rank`` (one entry per query):
    ``rank = 1 + greater + equal / 2`` (ties share the mean rank).  Returns a dict with ``mrr`` = mean(1 / rank),
    ``mean_rank``, ``hits@K`` = mean(rank <= K) for every K of ``ks``, ``auc`` = mean(1 - (greater + equal / 2) /
    candidates) over the queries that have a candidate (the exact per-source AUC against ALL filtered non-edges) and
    ``queries``.  A count of -1 (a query whose index was out of range) raises ValueError; no query gives NaN."""
    greater, equal, candidates = (torch.as_tensor(x).reshape(-1) for x in (greater, equal, candidates))
    if not (greater.numel() == equal.numel() == candidates.numel()):
        raise ValueError("rank_metrics: greater, equal and candidates must have one length")
    if any(bool((x < 0).any()) for x in (greater, equal, candidates)):
        raise ValueError("rank_metrics: a negative count (a query with an index outside [0, n))")
    m = greater.numel()
    out = {"queries": m}
    nan = float("nan")
    if m == 0:
        out.update(mrr=nan, mean_rank=nan, auc=nan, **{f"hits@{int(k)}": nan for k in ks})
        return out
    above = greater.double() + equal.double() / 2
    rank = 1 + above
    out["mrr"] = float((1 / rank).mean())
    out["mean_rank"] = float(rank.mean())
    for k in ks:
        out[f"hits@{int(k)}"] = float((rank <= k).double().mean())
    has = candidates > 0
    out["auc"] = float((1 - above[has] / candidates[has].double()).mean()) if bool(has.any()) else nan
    return out


def _csr_keys(indptr, indices, n, exclude_self):
    """the distinct keys i n + j of the entries (i, j) of a CSR with n rows, sorted: entries outside [0, n) ignored,
    the diagonal dropped under ``exclude_self``"""
    indptr = indptr.reshape(-1).long()
    rows = torch.repeat_interleave(torch.arange(n, device=indptr.device), indptr[1:] - indptr[:-1])
    cols = indices.reshape(-1).long()[int(indptr[0]):int(indptr[-1])] if n else indices.reshape(-1).long()[:0]
    keep = (cols >= 0) & (cols < n)
    if exclude_self:
        keep &= cols != rows
    return torch.unique(rows[keep] * n + cols[keep])


def reconstruction_metrics(pred_indptr, pred_index, true_indptr, true_indices, node_ptr=None, exclude_self=True):
    """How well a decoded graph (``GAE.reconstruct`` / ``ops.decoder_threshold``: CSR ``pred_indptr`` [n + 1],
    ``pred_index``) reproduces the graph it was decoded from (CSR ``true_indptr`` [n + 1], ``true_indices``), over the
    ordered pairs (i, j): plain torch ops on the device of ``pred_indptr``.  On either side the pairs are the distinct
    entries of the CSR -- a repeated entry counts once, entries outside [0, n) are ignored, the diagonal is dropped
    under ``exclude_self``.  Returns a dict: ``tp`` / ``fp`` / ``fn`` (ints), ``n_pred`` = tp + fp, ``precision`` =
    tp / n_pred, ``recall`` = tp / (tp + fn), ``f1`` = 2 tp / (2 tp + fp + fn); an empty denominator gives NaN.
    With ``node_ptr`` (int [G + 1] member offsets of a batched graph) also ``exact``, bool [G]: the predicted pairs of
    the member's rows are exactly its true pairs (an empty member is exact), and ``exact_fraction``, its mean (NaN when
    G = 0) -- the share of molecules whose bond graph is reproduced."""
    pred_indptr = torch.as_tensor(pred_indptr)
    dev = pred_indptr.device
    pred_index, true_indptr, true_indices = (torch.as_tensor(t, device=dev) for t in (pred_index, true_indptr, true_indices))
    n = pred_indptr.numel() - 1
    if n < 0 or true_indptr.numel() != n + 1:
        raise ValueError(f"reconstruction_metrics: row pointers of {pred_indptr.numel()} and {true_indptr.numel()} "
                         "entries: both must be [n + 1]")
    pred = _csr_keys(pred_indptr, pred_index, n, exclude_self)
    true = _csr_keys(true_indptr, true_indices, n, exclude_self)
    hit = torch.isin(pred, true, assume_unique=True)
    tp = int(hit.sum())
    n_pred, n_true = int(pred.numel()), int(true.numel())
    fp, fn = n_pred - tp, n_true - tp
    nan = float("nan")
    out = {"tp": tp, "fp": fp, "fn": fn, "n_pred": n_pred,
           "precision": tp / n_pred if n_pred else nan, "recall": tp / n_true if n_true else nan,
           "f1": 2 * tp / (n_pred + n_true) if n_pred + n_true else nan}
    if node_ptr is not None:
        node_ptr = torch.as_tensor(node_ptr, device=dev).reshape(-1).long()
        G = node_ptr.numel() - 1
        if G < 0:
            raise ValueError("reconstruction_metrics: node_ptr must be [G + 1]")
        wrong = torch.cat([pred[~hit], true[~torch.isin(true, pred, assume_unique=True)]])
        rows = torch.div(wrong, max(n, 1), rounding_mode="floor")
        member = torch.searchsorted(node_ptr, rows, right=True) - 1
        inside = (member >= 0) & (member < G)
        out["exact"] = torch.bincount(member[inside], minlength=max(G, 0))[:max(G, 0)] == 0
        out["exact_fraction"] = float(out["exact"].double().mean()) if G > 0 else nan
    return out


def graph_scores_dense(z_g, csr_g, exclude_self=True):
    """The per-graph scores of ``GAE.score_graphs`` / ``ops.score_graphs`` for ONE graph of any size, by the definitions
    taken literally with torch ops on the device of ``z_g`` [n, d]: the route of graphs above the fused kernel's 64
    nodes, and a cross-check of it.  ``csr_g`` = (indptr [n + 1], indices) of the graph alone, local column ids (entries
    outside [0, n) are ignored, a repeated entry is one positive).  Logits: the k-ascending chain from 0 of
    z_i[k] z_j[k], every step rounded to fp32 (through an exact fp64 product: the fmaf chain up to double rounding).
    Returns a dict of Python numbers: loss, auc, ap (NaN where a class is missing), n_pos, n_neg, wins, ties (-1, and
    NaN, when a logit is not finite)."""
    nan = float("nan")
    z = torch.as_tensor(z_g).detach().float()
    n, d = z.shape
    dev = z.device
    indptr, indices = (torch.as_tensor(t, device=dev).long() for t in csr_g)
    rows = torch.repeat_interleave(torch.arange(n, device=dev), indptr[1:] - indptr[:-1])
    cols = indices[int(indptr[0]):int(indptr[-1])]
    inside = (cols >= 0) & (cols < n)
    rows, cols = rows[inside], cols[inside]
    s = torch.zeros(n, n, dtype=torch.float32, device=dev)
    zd = z.double()
    for k in range(d):
        s = (s.double() + zd[:, k:k + 1] * zd[None, :, k]).float()
    if not bool(torch.isfinite(s).all()):
        return {"loss": nan, "auc": nan, "ap": nan, "n_pos": -1, "n_neg": -1, "wins": -1, "ties": -1}
    # the loss of train_inductive.py:44-48 on this graph alone: all n^2 pairs, y_ij = the number of entries j in row i
    y = torch.zeros(n * n, dtype=torch.float64, device=dev)
    y.index_put_((rows * n + cols,), torch.ones(rows.numel(), dtype=torch.float64, device=dev), accumulate=True)
    y = y.view(n, n)
    S = float(y.sum())
    x = s.double()
    sp = torch.nn.functional.softplus
    # the positives in CSR order, first occurrences
    keys = rows * n + cols
    if exclude_self:
        keys = keys[rows != cols]
    if keys.numel():
        uniq, inv = torch.unique(keys, return_inverse=True)
        first = torch.full((uniq.numel(),), keys.numel(), dtype=torch.long, device=dev)
        first.scatter_reduce_(0, inv, torch.arange(keys.numel(), device=dev), reduce="amin")
        keys = keys[torch.sort(first).values]
    flat = s.view(-1)
    member = torch.ones(n, n, dtype=torch.bool, device=dev)
    if exclude_self:
        member.fill_diagonal_(False)
    is_pos = torch.zeros(n * n, dtype=torch.bool, device=dev)
    is_pos[keys] = True
    P = flat[keys]
    Q = flat[member.view(-1) & ~is_pos]
    n_pos, n_neg = int(P.numel()), int(Q.numel())
    out = {"n_pos": n_pos, "n_neg": n_neg, "wins": 0, "ties": 0, "auc": nan, "ap": nan, "loss": nan}
    if n_pos > 0:
        pw = (float(n) * n - S) / S
        out["loss"] = float((sp(x) + y * ((pw - 1) * sp(-x) - x)).sum() / (float(n) * n))
    if n_pos > 0 and n_neg > 0:
        qs, ps = torch.sort(Q).values, torch.sort(P).values
        lo, hi = torch.searchsorted(qs, P, right=False), torch.searchsorted(qs, P, right=True)
        out["wins"], out["ties"] = int(lo.sum()), int((hi - lo).sum())
        out["auc"] = (out["wins"] + out["ties"] / 2) / (float(n_pos) * n_neg)
        pos_ge = n_pos - torch.searchsorted(ps, P, right=False)
        all_ge = pos_ge + (n_neg - lo)
        out["ap"] = float((pos_ge.double() / all_ge.double()).sum() / n_pos)
    return out


def graph_score_summary(scores):
    """What a set of per-graph scores says in a few numbers.  ``scores``: a ``GraphScores`` (or anything with auc, ap,
    loss, n_pos, n_neg, wins, ties of one length).  Over the graphs that have both classes (n_pos > 0 and n_neg > 0;
    refused graphs carry -1): the means ``auc``, ``ap``, ``loss``; ``micro_auc`` = (sum wins + sum ties / 2) / sum
    n_pos n_neg -- every (positive, negative) pair of the set weighs the same; ``graphs`` = how many they are,
    ``left_out`` = the others.  NaN when no graph has both classes."""
    n_pos, n_neg, wins, ties = (torch.as_tensor(getattr(scores, k)).reshape(-1).long()
                                for k in ("n_pos", "n_neg", "wins", "ties"))
    auc, ap, loss = (torch.as_tensor(getattr(scores, k)).reshape(-1).double() for k in ("auc", "ap", "loss"))
    both = (n_pos > 0) & (n_neg > 0)
    m = int(both.sum())
    out = {"graphs": m, "left_out": int(both.numel()) - m}
    nan = float("nan")
    if m == 0:
        out.update(auc=nan, ap=nan, loss=nan, micro_auc=nan)
        return out
    out["auc"] = float(auc[both].mean())
    out["ap"] = float(ap[both].mean())
    out["loss"] = float(loss[both].mean())
    pairs = float((n_pos[both].double() * n_neg[both].double()).sum())
    out["micro_auc"] = (float(wins[both].double().sum()) + float(ties[both].double().sum()) / 2) / pairs
    return out


def clustering_metrics(pred, true):
    """How well cluster labels ``pred`` [n] agree with classes ``true`` [n] (rows with ``true < 0`` are ignored): a
    dict with ``nmi`` (mutual information over the ARITHMETIC mean of the two entropies, natural logarithms), ``ari``
    (adjusted Rand index from the contingency table), ``acc`` (the best one-to-one matching of clusters to classes,
    scipy.optimize.linear_sum_assignment) and ``n`` (rows counted).  Host code on the small contingency table.  Two
    single-cluster labellings agree perfectly (1 / 1 / 1); no row gives NaN."""
    pred, true = np.asarray(pred).reshape(-1), np.asarray(true).reshape(-1)
    if pred.shape != true.shape:
        raise ValueError(f"clustering_metrics: {pred.size} predictions for {true.size} labels")
    keep = true >= 0
    pred, true = pred[keep], true[keep]
    n = int(pred.size)
    nan = float("nan")
    if n == 0:
        return {"nmi": nan, "ari": nan, "acc": nan, "n": 0}
    _, pi = np.unique(pred, return_inverse=True)
    _, ti = np.unique(true, return_inverse=True)
    table = np.zeros((int(pi.max()) + 1, int(ti.max()) + 1), dtype=np.int64)
    np.add.at(table, (pi, ti), 1)
    a, b = table.sum(1).astype(np.float64), table.sum(0).astype(np.float64)
    # NMI
    nz = table > 0
    p = table[nz] / n
    mi = float((p * np.log(p / (np.outer(a, b)[nz] / (float(n) * n)))).sum())
    ha = float(-(a / n * np.log(a / n)).sum())
    hb = float(-(b / n * np.log(b / n)).sum())
    nmi = 1.0 if ha + hb == 0 else max(mi, 0.0) / ((ha + hb) / 2)
    # ARI
    comb = lambda x: x * (x - 1) / 2.0
    sum_ij, sum_a, sum_b = float(comb(table.astype(np.float64)).sum()), float(comb(a).sum()), float(comb(b).sum())
    expected = sum_a * sum_b / comb(float(n)) if n > 1 else 0.0
    upper = (sum_a + sum_b) / 2
    ari = 1.0 if upper == expected else (sum_ij - expected) / (upper - expected)
    # accuracy under the best one-to-one matching
    from scipy.optimize import linear_sum_assignment
    rows, cols = linear_sum_assignment(-table)
    return {"nmi": float(nmi), "ari": float(ari), "acc": float(table[rows, cols].sum()) / n, "n": n}


KNN_DISTANCE_EPS = 1e-12


def knn_predict(index, value, y, *, task="regression", weights="uniform", n_classes=None):
    """The kNN regressor / classifier over neighbour lists: ``index`` [m, k] (rows of the database, -1 = padding) and
    ``value`` [m, k] as ``ops.knn`` returns them, ``y`` [n] the targets of the database rows.  Torch on the device of
    ``index``; no m x n matrix.
    ``task="regression"``: fp64 [m], the mean of the neighbours' targets, or under ``weights="distance"`` their mean
    weighted by 1 / (sqrt(value) + 1e-12) (``value`` = the squared distances of metric "l2"); a NaN target does not
    vote; a row with no voter is NaN.
    ``task="classification"``: int64 [m], the class with the most (or, weighted, the heaviest) votes among the
    neighbours' labels in [0, n_classes) (default: max label + 1), ties to the LOWER class; a neighbour whose label is
    -1 (unlabelled) does not vote; a row with no voter is -1.
    With the lists of a self-search (``ops.knn(Z, k=k)``: every row left out of its own list) this is the
    leave-one-out prediction."""
    if task not in ("regression", "classification"):
        raise ValueError(f"task: 'regression' or 'classification', not {task!r}")
    if weights not in ("uniform", "distance"):
        raise ValueError(f"weights: 'uniform' or 'distance', not {weights!r}")
    index = torch.as_tensor(index)
    dev = index.device
    value = torch.as_tensor(value).to(dev)
    y = torch.as_tensor(y).to(dev).reshape(-1)
    if index.dim() != 2 or value.shape != index.shape:
        raise ValueError(f"knn_predict: index {tuple(index.shape)} and value {tuple(value.shape)} must be equal [m, k]")
    idx = index.long()
    if idx.numel() and int(idx.max()) >= y.numel():
        raise ValueError(f"knn_predict: a neighbour index {int(idx.max())} beyond the {y.numel()} targets")
    votes = idx >= 0
    if y.numel() == 0:
        y = torch.zeros(1, dtype=y.dtype, device=dev)          # every entry is padding: nothing is gathered for real
    got = y[idx.clamp(min=0)]
    if weights == "distance":
        w = 1.0 / (value.double().clamp(min=0.0).sqrt() + KNN_DISTANCE_EPS)
    else:
        w = torch.ones(idx.shape, dtype=torch.float64, device=dev)
    if task == "regression":
        got = got.double()
        votes = votes & ~torch.isnan(got)
        w = torch.where(votes, w, torch.zeros_like(w))
        total = w.sum(1)
        pred = (w * torch.where(votes, got, torch.zeros_like(got))).sum(1) / total
        return torch.where(total > 0, pred, torch.full_like(pred, float("nan")))
    if got.is_floating_point():
        raise ValueError("knn_predict: classification takes integer labels")
    got = got.long()
    votes = votes & (got >= 0)
    C = int(n_classes) if n_classes is not None else (int(y.max()) + 1 if y.numel() else 0)
    C = max(C, 1)
    if bool((got[votes] >= C).any()):
        raise ValueError(f"knn_predict: a label beyond n_classes = {C}")
    w = torch.where(votes, w, torch.zeros_like(w))
    score = torch.zeros(idx.shape[0], C, dtype=torch.float64, device=dev)
    score.scatter_add_(1, torch.where(votes, got, torch.zeros_like(got)), w)
    best = score.max(1, keepdim=True).values
    classes = torch.arange(C, device=dev).expand_as(score)
    pred = torch.where(score == best, classes, torch.full_like(classes, C)).min(1).values     # ties: the lower class
    return torch.where(votes.any(1), pred, torch.full_like(pred, -1))


def neighbourhood_preservation(index_a, index_b, chunk_rows=65536):
    """mean, over the rows, of the fraction of a row's neighbours in ``index_a`` [n, k] that are also among its
    neighbours in ``index_b`` [n, k'] -- two ``ops.knn`` index tables of the same rows in two spaces (an embedding and
    its 2-D map): 1.0 when every neighbourhood survives, about k' / n for unrelated spaces.  Entries of -1 are padding;
    a row without neighbours in ``index_a`` is left out (NaN when every row is).  No n x n matrix and no ranks: the
    tables are compared k x k' per row, in chunks of ``chunk_rows`` rows.  Torch on the device of ``index_a``; a Python
    number out."""
    a = torch.as_tensor(index_a)
    b = torch.as_tensor(index_b).to(a.device)
    if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[0]:
        raise ValueError(f"neighbourhood_preservation: two [n, k] index tables of the same rows, got {tuple(a.shape)} and "
                         f"{tuple(b.shape)}")
    total, rows = 0.0, 0
    for r0 in range(0, a.shape[0], int(chunk_rows)):
        x, y = a[r0:r0 + chunk_rows].long(), b[r0:r0 + chunk_rows].long()
        valid = x >= 0
        hit = ((x.unsqueeze(2) == y.unsqueeze(1)).any(2) & valid).sum(1).double()
        cnt = valid.sum(1)
        keep = cnt > 0
        total += float((hit[keep] / cnt[keep].double()).sum())
        rows += int(keep.sum())
    return total / rows if rows else float("nan")


def regression_metrics(pred, y):
    """``rmse``, ``mae``, ``r2`` (1 - SSE / SST about the mean of the scored targets; NaN when they are constant) and ``n``
    of predictions ``pred`` [m] against targets ``y`` [m], as the reference's chemistry table reports them (README.md:
    "GAE + Ridge / MLP / Random Forest").  Rows whose prediction or target is NaN (``knn_predict``: no voter) are left
    out and counted in ``left_out``.  Torch on the device of ``pred``, fp64; Python numbers out."""
    pred = torch.as_tensor(pred).double().reshape(-1)
    y = torch.as_tensor(y).to(pred.device).double().reshape(-1)
    if pred.shape != y.shape:
        raise ValueError(f"regression_metrics: {pred.numel()} predictions for {y.numel()} targets")
    keep = ~(torch.isnan(pred) | torch.isnan(y))
    n = int(keep.sum())
    nan = float("nan")
    if n == 0:
        return {"rmse": nan, "mae": nan, "r2": nan, "n": 0, "left_out": int(pred.numel())}
    p, t = pred[keep], y[keep]
    err = p - t
    sse = float((err * err).sum())
    sst = float(((t - t.mean()) ** 2).sum())
    return {"rmse": (sse / n) ** 0.5, "mae": float(err.abs().mean()), "r2": 1.0 - sse / sst if sst > 0 else nan, "n": n,
            "left_out": int(pred.numel()) - n}


def classification_metrics(pred, true, proba=None, n_classes=None):
    """``accuracy``, ``macro_f1``, per-class ``precision`` / ``recall`` / ``f1`` (lists, 0 where the denominator is 0), the
    ``confusion`` matrix (int64 [c, c] as nested lists: row = true class, column = predicted class) and ``n`` of class
    predictions ``pred`` [m] against classes ``true`` [m]; with ``proba`` [m, c] also ``log_loss`` (the mean of -log of
    the true class's probability, clipped at 1e-15) and, for two classes, ``roc_auc`` of column 1.  Rows whose true label
    is -1 are not scored; a scored row whose prediction is -1 (``LogRegResult.predict``: a non-finite row) counts as an
    error in ``accuracy`` and the recalls, is in no column of the matrix, is left out of the probability scores and is
    counted in ``unpredicted``.  Torch on the device of ``pred``, fp64; Python numbers out."""
    pred = torch.as_tensor(pred).long().reshape(-1)
    true = torch.as_tensor(true).to(pred.device).long().reshape(-1)
    if pred.shape != true.shape:
        raise ValueError(f"classification_metrics: {pred.numel()} predictions for {true.numel()} labels")
    hi = int(max(pred.max(), true.max())) if pred.numel() else -1
    c = hi + 1 if n_classes is None else int(n_classes)
    if proba is not None:
        proba = torch.as_tensor(proba).to(pred.device).double()
        if proba.dim() != 2 or proba.shape[0] != pred.numel():
            raise ValueError(f"classification_metrics: proba must be [{pred.numel()}, c], got {tuple(proba.shape)}")
        c = max(c, proba.shape[1]) if n_classes is None else c
        if proba.shape[1] != c:
            raise ValueError(f"classification_metrics: proba has {proba.shape[1]} columns for {c} classes")
    if c < 1 or hi >= c or (pred.numel() and int(min(pred.min(), true.min())) < -1):
        raise ValueError(f"classification_metrics: labels must lie in -1..{c - 1}")
    scored = true >= 0
    n = int(scored.sum())
    nan = float("nan")
    t, p = true[scored], pred[scored]
    seen = p >= 0
    conf = torch.bincount(t[seen] * c + p[seen], minlength=c * c).reshape(c, c)
    tp = conf.diagonal().double()
    support, called = torch.bincount(t, minlength=c).double(), conf.sum(0).double()
    zero = torch.zeros_like(tp)
    precision = torch.where(called > 0, tp / called.clamp_min(1), zero)
    recall = torch.where(support > 0, tp / support.clamp_min(1), zero)
    f1 = torch.where(precision + recall > 0, 2 * precision * recall / (precision + recall).clamp_min(1e-300), zero)
    present = support > 0                                               # macro-F1 over the classes that occur
    out = {"accuracy": float(tp.sum()) / n if n else nan, "macro_f1": float(f1[present].mean()) if n else nan,
           "precision": precision.tolist(), "recall": recall.tolist(), "f1": f1.tolist(), "confusion": conf.tolist(),
           "n": n, "unpredicted": int((~seen).sum())}
    if proba is not None:
        P = proba[scored][seen]
        ts = t[seen]
        ok = ~torch.isnan(P).any(1)
        P, ts = P[ok], ts[ok]
        out["log_loss"] = float(-torch.log(P.gather(1, ts[:, None]).clamp_min(1e-15)).mean()) if P.shape[0] else nan
        if c == 2:
            pos, neg = P[ts == 1, 1], P[ts == 0, 1]
            out["roc_auc"] = roc_auc(pos, neg) if pos.numel() and neg.numel() else nan
    return out
