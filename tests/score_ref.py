"""numpy fp64 reference of gae_score_graphs (K20) for the tests: the definitions of include/gae_hip_experimental.h taken
literally, counts by brute force over all (positive, negative) pairs -- plus the fixtures both the CPU and the GPU tests
use (so the CPU file can check a fixture's own suitability with the oracle alone)."""
import numpy as np

INT_BOUND = float(2 ** 24)          # integers below it are exact in fp32, sums and products included


def csr_rows(n_rows, rows, cols):
    """(indptr int32, indices int32) of the entries (rows[e], cols[e]); the entries of a row keep their given order"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    order = np.argsort(rows, kind="stable")
    indptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.add.at(indptr, rows + 1, 1)
    return np.cumsum(indptr).astype(np.int32), cols[order].astype(np.int32)


def graph_entries(indptr, indices, r0, n):
    """the entries of rows [r0, r0 + n) with a column inside them, in CSR order: local (i, j) arrays"""
    e0, e1 = int(indptr[r0]), int(indptr[r0 + n])
    rows = np.repeat(np.arange(n), np.diff(np.asarray(indptr[r0:r0 + n + 1], dtype=np.int64)))
    cols = np.asarray(indices[e0:e1], dtype=np.int64) - r0
    inside = (cols >= 0) & (cols < n)
    return rows[inside], cols[inside]


def scores_from_logits(s, indptr, indices, r0, n, exclude_self=True):
    """the outputs of one graph from its [n, n] logits ``s``: dict with n_pos, n_neg, wins, ties, auc, ap, loss and the
    score lists pos (CSR order, first occurrences) / neg"""
    nan = float("nan")
    s = np.asarray(s, dtype=np.float64).reshape(n, n)
    rows, cols = graph_entries(indptr, indices, r0, n)
    y = np.zeros((n, n))
    np.add.at(y, (rows, cols), 1.0)
    seen, pos_keys = set(), []
    for i, j in zip(rows.tolist(), cols.tolist()):
        if (exclude_self and i == j) or (i, j) in seen:
            continue
        seen.add((i, j))
        pos_keys.append((i, j))
    is_pos = np.zeros((n, n), dtype=bool)
    for i, j in pos_keys:
        is_pos[i, j] = True
    member = np.ones((n, n), dtype=bool)
    if exclude_self:
        np.fill_diagonal(member, False)
    P = np.array([s[i, j] for i, j in pos_keys], dtype=np.float64)
    Q = s[member & ~is_pos]
    n_pos, n_neg = len(P), len(Q)
    out = {"n_pos": n_pos, "n_neg": n_neg, "wins": 0, "ties": 0, "auc": nan, "ap": nan, "loss": nan, "pos": P, "neg": Q}
    if not np.isfinite(s).all():
        out.update(n_pos=-1, n_neg=-1, wins=-1, ties=-1)
        return out
    if n_pos > 0:
        S = y.sum()
        pw = (float(n) * n - S) / S
        sp = lambda v: np.logaddexp(0.0, v)          # noqa: E731
        out["loss"] = float((sp(s) + y * ((pw - 1) * sp(-s) - s)).sum() / (float(n) * n))
    if n_pos > 0 and n_neg > 0:
        out["wins"] = int((P[:, None] > Q[None, :]).sum())
        out["ties"] = int((P[:, None] == Q[None, :]).sum())
        out["auc"] = (out["wins"] + out["ties"] / 2) / (float(n_pos) * n_neg)
        both = np.concatenate([P, Q])
        ap = 0.0
        for p in P:                                  # CSR order, one fp64 chain
            ap += float((P >= p).sum()) / float((both >= p).sum())
        out["ap"] = ap / n_pos
    return out


def graph_scores(Z, indptr, indices, r0, n, exclude_self=True):
    """the outputs of the graph with rows [r0, r0 + n) for the embedding Z [N, d] (logits in fp64)"""
    Zg = np.asarray(Z, dtype=np.float64)[r0:r0 + n]
    return scores_from_logits(Zg @ Zg.T, indptr, indices, r0, n, exclude_self)


def band(s, indptr, indices, r0, n, delta, exclude_self=True):
    """what a logit error of at most ``delta`` per pair leaves open: a comparison s_p ? s_q can only come out otherwise
    when |s_p - s_q| <= 2 delta.  lo = #(s_p - s_q > 2 delta), hi = #(s_p - s_q >= -2 delta) bound wins from below and
    wins + ties from above; ap_lo / ap_hi apply the same shift to every comparison of the AP terms
    pos_ge / (pos_ge + neg_ge) (increasing in pos_ge, decreasing in neg_ge)."""
    ref = scores_from_logits(s, indptr, indices, r0, n, exclude_self)
    P, Q = ref["pos"], ref["neg"]
    out = dict(ref, lo=0, hi=0, ap_lo=float("nan"), ap_hi=float("nan"))
    if len(P) and len(Q):
        diff = P[:, None] - Q[None, :]
        out["lo"], out["hi"] = int((diff > 2 * delta).sum()), int((diff >= -2 * delta).sum())
        pp = P[None, :] - P[:, None]                 # [p, p']: s_p' - s_p
        qp = Q[None, :] - P[:, None]
        other = ~np.eye(len(P), dtype=bool)          # p itself always counts
        pge_lo, pge_hi = ((pp >= 2 * delta) & other).sum(1) + 1, ((pp >= -2 * delta) & other).sum(1) + 1
        nge_lo, nge_hi = (qp > 2 * delta).sum(1), (qp >= -2 * delta).sum(1)
        out["ap_lo"] = float((pge_lo / (pge_lo + nge_hi)).mean())
        out["ap_hi"] = float((pge_hi / (pge_hi + nge_lo)).mean())
    return out


def encode_graph(X, y, Ws, bs, norm="none", integers=False):
    """fp64 GCN encoder of gae.py:26-31,36-45 on one graph: X [n, f], y [n, n] entry counts (row = destination), ReLU on
    all but the last layer.  ``integers``: assert that every intermediate is an integer below 2^24 (then fp32 computes
    it exactly, in any order)"""
    H = np.asarray(X, dtype=np.float64)
    deg = y.sum(1)
    sc = np.where(deg > 0, 1.0 / np.sqrt(np.maximum(deg, 1)), 0.0)

    def check(v):
        if integers:
            assert np.all(v == np.round(v)) and (np.abs(v).max() if v.size else 0) < INT_BOUND
    for l, (W, b) in enumerate(zip(Ws, bs)):
        M = sc[:, None] * (y @ (sc[:, None] * H)) if norm == "both" else y @ H
        check(M)
        if integers:                                 # every partial sum of a product chain, whatever its order
            assert (np.abs(M) @ np.abs(np.asarray(W, dtype=np.float64)).T).max(initial=0) + 1 < INT_BOUND
        H = M @ np.asarray(W, dtype=np.float64).T + (0 if b is None else np.asarray(b, dtype=np.float64))
        check(H)
        if l < len(Ws) - 1:
            H = np.maximum(H, 0)
    if integers and H.size:
        assert (np.abs(H) @ np.abs(H).T).max() < INT_BOUND
    return H


def set_scores(gp, indptr, indices, X, Ws, bs, norm="none", exclude_self=True, integers=False):
    """encode_graph + graph_scores of every graph of a set; returns (list of dicts, list of logit matrices)"""
    rows, logits = [], []
    for g in range(len(gp) - 1):
        r0, n = int(gp[g]), int(gp[g + 1] - gp[g])
        i, j = graph_entries(indptr, indices, r0, n)
        y = np.zeros((n, n))
        np.add.at(y, (i, j), 1.0)
        Z = encode_graph(np.asarray(X)[r0:r0 + n], y, Ws, bs, norm, integers)
        s = Z @ Z.T
        logits.append(s)
        rows.append(scores_from_logits(s, indptr, indices, r0, n, exclude_self))
    return rows, logits


# ---------------------------------------------------------------------------------------------------------- fixtures
def molecule_set(rng, sizes, directed=False):
    """(gp, rows, cols): a random tree per graph plus a few extra bonds, both directions; ``directed``: random directed
    entries with repeats and self loops instead.  rows = destination, cols = source, global ids"""
    sizes = np.asarray(sizes, dtype=np.int64)
    gp = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(sizes, out=gp[1:])
    rows, cols = [], []
    for g, n in enumerate(sizes.tolist()):
        if n == 0 or (n < 2 and not directed):
            continue
        if directed:
            e = int(rng.integers(0, 3 * n + 1))
            a, b = rng.integers(0, n, e), rng.integers(0, n, e)
            if e > 4:
                a[:2] = a[2:4]; b[:2] = b[2:4]       # repeated entries
                a[4] = b[4]                           # a self loop
        else:
            child = np.arange(1, n)
            parent = child - np.minimum(rng.integers(1, 4, n - 1), child)
            extra = int(rng.integers(0, 4))
            u = np.concatenate([child, rng.integers(0, n, extra)]); v = np.concatenate([parent, rng.integers(0, n, extra)])
            keep = u != v
            u, v = u[keep], v[keep]
            a = np.stack([u, v], 1).reshape(-1); b = np.stack([v, u], 1).reshape(-1)
        rows.append(a + gp[g]); cols.append(b + gp[g])
    cat = lambda xs: np.concatenate(xs).astype(np.int64) if xs else np.zeros(0, np.int64)      # noqa: E731
    return gp, cat(rows), cat(cols)


def integer_encoder(rng, f_in, hidden, density=0.3):
    """weights and biases in {-1, 0, 1}, mostly zero"""
    Ws, bs, prev = [], [], f_in
    for h in hidden:
        Ws.append((rng.integers(-1, 2, (h, prev)) * (rng.random((h, prev)) < density)).astype(np.float32))
        bs.append((rng.integers(-1, 2, h) * (rng.random(h) < density)).astype(np.float32))
        prev = h
    return Ws, bs


def integer_fixture(hidden, n_graphs=400, seed=17):
    """item 2's fixture: 0 / 1 features, weights and biases in {-1, 0, 1}"""
    rng = np.random.default_rng(seed + len(hidden))
    gp, rows, cols = molecule_set(rng, rng.integers(1, 40, n_graphs))
    X = (rng.random((int(gp[-1]), 39)) < 0.15).astype(np.float32)
    Ws, bs = integer_encoder(rng, 39, hidden)
    return gp, rows, cols, X, Ws, bs


def band_fixture(seed=5, n_graphs=300, f_in=39, hidden=(32, 16)):
    """item 3's fixture: ZINC-sized molecules, seeded continuous fp32 features (one-hot rows would give symmetric atoms
    the same embedding, hence ties), general weights"""
    rng = np.random.default_rng(seed)
    gp, rows, cols = molecule_set(rng, rng.integers(6, 39, n_graphs))
    X = rng.standard_normal((int(gp[-1]), f_in)).astype(np.float32)
    Ws, bs, prev = [], [], f_in
    for h in hidden:
        k = 1.0 / np.sqrt(prev)
        Ws.append(rng.uniform(-k, k, (h, prev)).astype(np.float32))
        bs.append(rng.uniform(-0.5, 0.5, h).astype(np.float32))
        prev = h
    return gp, rows, cols, X, Ws, bs


def band_totals(gp, indptr, indices, logits, exclude_self=True):
    """(per-graph band dicts, delta, sum of hi - lo, sum of n_pos n_neg) of a fixture's oracle logits"""
    delta = 1e-5 * max(float(np.abs(s).max()) for s in logits if s.size)
    rows = [band(s, indptr, indices, int(gp[g]), int(gp[g + 1] - gp[g]), delta, exclude_self)
            for g, s in enumerate(logits)]
    open_pairs = sum(r["hi"] - r["lo"] for r in rows)
    pairs = sum(r["n_pos"] * r["n_neg"] for r in rows)
    return rows, delta, open_pairs, pairs
