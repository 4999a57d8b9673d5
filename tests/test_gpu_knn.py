"""K24 on the device (gae_knn, ops.knn, GAE.nearest_nodes / nearest_graphs, metrics.knn_predict, the two scripts) against
the fp64 brute force tests/knn_ref.py.  Shapes are the smallest at which each mechanism can break: one panel and panel
tails (m = 1, 31, 33, 65), one and several blocks of four panels, tile tails (n = 1 .. 65, 130), several tiles per split
and several splits (n = 2708), every DH form of the product tile and the chunked form (d <= 16, <= 32, <= 64, > 64),
k = 1, k > n and the largest k."""
import os

import numpy as np
import pytest
import torch

import knn_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def as_np(t):
    return t.detach().cpu().numpy()


def strided(X, pad, dev):
    """X [n, d] on the device as a view of a [n, d + pad] buffer whose pad columns hold NaN: never read as data"""
    X = torch.as_tensor(X, dtype=torch.float32)
    buf = torch.full((X.shape[0], X.shape[1] + pad), NAN, dtype=torch.float32)
    buf[:, :X.shape[1]] = X
    return buf.to(dev)[:, :X.shape[1]]


def raw_knn(Q, X, k, metric, flags=0, splits=0, pad=3):
    """gae_knn on device tensors (strided views allowed) into outputs with ldo = k + pad; the pad columns are checked to
    be untouched.  Returns (index int32 [m, k], value fp32 [m, k]) on the host"""
    from gae_dgl_amd import _lib
    from gae_dgl_amd.ops import _ptr, _stream
    m, d = Q.shape
    n = X.shape[0]
    ldq = Q.stride(0) if m > 1 else d
    ldx = X.stride(0) if n > 1 else d
    nbytes = _lib.load().gae_knn_workspace_bytes(m, n, d, k, splits)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=Q.device)
    index = torch.full((m, k + pad), -7, dtype=torch.int32, device=Q.device)
    value = torch.full((m, k + pad), NAN, dtype=torch.float32, device=Q.device)
    _lib.call("gae_knn", _ptr(Q), ldq, m, _ptr(X), ldx, n, d, k, {"l2": 0, "dot": 1}[metric], flags, splits, _ptr(index),
              _ptr(value), k + pad, _ptr(ws), ws.numel(), _stream())
    torch.cuda.synchronize()
    assert bool((index[:, k:] == -7).all()) and bool(torch.isnan(value[:, k:]).all()), "a store beyond k"
    return as_np(index[:, :k]), as_np(value[:, :k])


def grid(rng, n, d):
    """multiples of 1/4 in [-4, 4]: at d <= 256 every product, h, key and direct distance is exact in fp32 (in units of
    1/16 the largest sum is 256 * 64 * 16 = 2^18 < 2^24)"""
    return (rng.integers(-16, 17, (n, d)) / 4.0).astype(np.float32)


# ------------------------------------------------------------------ 1. bit for bit on an exact grid
MS, NS, DS, KS = [1, 31, 33, 65], [1, 2, 31, 32, 33, 63, 64, 65, 130, 2708], [1, 3, 16, 17, 48, 64, 65, 192, 256], [1, 5, 64]
GRID_CASES = sorted({(MS[i % 4], NS[i % 10], DS[i % 9], KS[(i // 3) % 3]) for i in range(36)}
                    | {(65, 2708, 256, 64), (33, 2708, 64, 64), (129, 2708, 1, 5), (257, 130, 48, 64)})


def test_the_grid_cases_cover_every_value_of_every_axis():
    for axis, values in enumerate((MS, NS, DS, KS)):
        assert set(values) <= {c[axis] for c in GRID_CASES}


@pytest.mark.parametrize("m, n, d, k", GRID_CASES)
def test_exact_on_a_grid(dev, m, n, d, k):
    rng = np.random.default_rng(m * 1000003 + n * 1009 + d * 17 + k)
    Q, X = grid(rng, m, d), grid(rng, n, d)
    Qd, Xd = strided(Q, 5, dev), strided(X, 2, dev)
    for metric in ("l2", "dot"):
        want_i, want_v = R.knn(Q, X, k, metric)
        for splits in (0, 2):
            got_i, got_v = raw_knn(Qd, Xd, k, metric, splits=splits)
            assert np.array_equal(got_i, want_i), (metric, splits, np.argwhere(got_i != want_i)[:4])
            assert np.array_equal(got_v.astype(np.float64), want_v), (metric, splits)


@pytest.mark.parametrize("n, d, k", [(65, 3, 5), (300, 1, 64), (2708, 16, 5), (130, 65, 64)])
def test_exact_self_search_with_duplicate_rows(dev, n, d, k):
    """a duplicate is a neighbour at distance exactly 0, and the row itself is absent"""
    rng = np.random.default_rng(n + d)
    X = grid(rng, n, d)
    X[n // 2:] = X[:n - n // 2]                                        # every row of the first half has a twin
    Xd = strided(X, 1, dev)
    for metric in ("l2", "dot"):
        want_i, want_v = R.knn(X, X, k, metric, exclude_same=True)
        got_i, got_v = raw_knn(Xd, Xd, k, metric, flags=1)
        assert np.array_equal(got_i, want_i) and np.array_equal(got_v.astype(np.float64), want_v), metric
        assert not (got_i == np.arange(n)[:, None]).any()
        if metric == "l2":
            assert (got_v[:, 0] == 0.0).sum() >= n - 1                 # (n odd: one row has no twin)


def test_empty_database_and_empty_query_set(dev):
    Q = torch.randn(5, 8, device=dev)
    i, v = raw_knn(Q, torch.empty(0, 8, device=dev), 3, "l2")
    assert (i == -1).all() and (v == INF).all()
    i, v = raw_knn(Q, torch.empty(0, 8, device=dev), 3, "dot")
    assert (i == -1).all() and (v == -INF).all()
    i, v = raw_knn(torch.empty(0, 8, device=dev), Q, 3, "l2")
    assert i.shape == (0, 3)


# ------------------------------------------------------------------ 2. the same chain as K16
@pytest.mark.parametrize("d", [16, 64, 200])
def test_dot_has_the_bits_of_decoder_topk(dev, d):
    from gae_dgl_amd import ops
    torch.manual_seed(d)
    Z = torch.randn(2708, d, device=dev)
    for k in (1, 10, 64):
        score, index = ops.decoder_topk(Z, k, exclude_edges=False)
        res = ops.knn(Z, k=k, metric="dot")
        assert res.index.dtype == torch.int32 and res.value.dtype == torch.float32
        assert torch.equal(res.index.long(), index)
        assert torch.equal(res.value.view(torch.int32), score.view(torch.int32))


# ------------------------------------------------------------------ 3. / 4. random data against fp64
RANDOM_SHAPES = [(4096, 20000, 48, 10), (1000, 5000, 192, 64)]


@pytest.fixture(scope="module", params=RANDOM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def random_case(request):
    m, n, d, k = request.param
    rng = np.random.default_rng(d)
    return rng.standard_normal((m, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32), k


def test_random_data_within_the_derived_tolerance(dev, random_case):
    from gae_dgl_amd import ops
    Q, X, k = random_case
    res = ops.knn(torch.from_numpy(Q).to(dev), torch.from_numpy(X).to(dev), k=k)
    bad = R.check_tolerant(Q, X, as_np(res.index), as_np(res.value))
    assert bad == [], bad[:5]


def test_the_reported_distance_is_the_direct_one(dev, random_case):
    """a common offset of +20 on every feature (a sum readout looks like this): the expanded form would lose the
    distance to cancellation (tests/test_knn_cpu.py shows it does); the reported value keeps the direct chain's bound"""
    from gae_dgl_amd import ops
    Q, X, k = random_case
    Q, X = (Q + np.float32(20)), (X + np.float32(20))
    d = Q.shape[1]
    res = ops.knn(torch.from_numpy(Q).to(dev), torch.from_numpy(X).to(dev), k=k)
    idx, val = as_np(res.index), as_np(res.value).astype(np.float64)
    assert (idx >= 0).all()
    D = R.pair_values(Q, X, idx, "l2")
    err, bound = np.abs(val - D), 2 * (d + 2) * 2.0 ** -24 * D + 1e-30
    print(f"max |value - D| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all(), float((err / bound).max())
    assert (np.diff(val, axis=1) >= 0).all()
    assert R.check_tolerant(Q, X, idx, val) == []


# ------------------------------------------------------------------ 5. schedule independence
def test_same_bits_for_any_split_stride_and_run(dev):
    from gae_dgl_amd import ops
    rng = np.random.default_rng(5)
    Q, X = rng.standard_normal((700, 17)).astype(np.float32), rng.standard_normal((5000, 17)).astype(np.float32)
    Qd, Xd = torch.from_numpy(Q).to(dev), torch.from_numpy(X).to(dev)
    for metric in ("l2", "dot"):
        base = ops.knn(Qd, Xd, k=7, metric=metric)
        runs = [ops.knn(Qd, Xd, k=7, metric=metric, splits=s) for s in (1, 3, 16)]
        runs.append(ops.knn(strided(Q, 11, dev), strided(X, 4, dev), k=7, metric=metric))
        wide = torch.zeros(700, 40, device=dev)
        wide[:, 3:20] = Qd
        runs.append(ops.knn(wide[:, 3:20], Xd, k=7, metric=metric, splits=5))      # read in place: ldq = 40, offset 3
        runs.append(ops.knn(Qd.t().contiguous().t(), Xd, k=7, metric=metric))       # inner stride != 1: copied
        runs.append(ops.knn(Qd, Xd, k=7, metric=metric))
        for r in runs:
            assert torch.equal(r.index, base.index), metric
            assert torch.equal(r.value.view(torch.int32), base.value.view(torch.int32)), metric
    self0 = ops.knn(Xd, k=7)
    for s in (1, 3, 16):
        r = ops.knn(Xd, k=7, splits=s)
        assert torch.equal(r.index, self0.index) and torch.equal(r.value, self0.value)


def test_short_lists_merge_the_same_for_any_split(dev):
    """the merge of the lane halves and of the column splits (topk_heap.h) on lists shorter than k: 60 of the 70 database
    rows are finite at k = 64; n = 70 is two full tiles and a tail of 6, m = 33 a panel and a tail of 1.  On the exact
    grid every split count must give the reference's bits, padding included"""
    rng = np.random.default_rng(70)
    m, n, d, k = 33, 70, 3, 64
    Q, X = grid(rng, m, d), grid(rng, n, d)
    X[[0, 5, 31, 32, 33, 40, 63, 64, 66, 69]] = NAN
    Qd, Xd = strided(Q, 5, dev), strided(X, 2, dev)
    for metric, pad in (("l2", INF), ("dot", -INF)):
        want_i, want_v = R.knn(Q, X, k, metric)
        # the reference alone: 60 neighbours per query, then -1 / +inf (l2), -1 / -inf (dot)
        assert (want_i[:, :60] >= 0).all() and (want_i[:, 60:] == -1).all() and (want_v[:, 60:] == pad).all()
        for splits in (1, 3, 16):
            got_i, got_v = raw_knn(Qd, Xd, k, metric, splits=splits)
            assert np.array_equal(got_i, want_i), (metric, splits)
            assert np.array_equal(got_v.astype(np.float64), want_v), (metric, splits)


@pytest.mark.parametrize("k", [5, 64])
@pytest.mark.parametrize("n", [1, 17, 33])
def test_more_splits_than_tiles(dev, n, k):
    """16 column splits over a database of one or two tiles of 32 rows: the parts are whole tiles, so all but one or two
    of them are empty (pb = pe = n) and their blocks write lists of padding alone; at k = 64 no query has k candidates.
    On the exact grid every call must give the reference's bits, and so the bits of one split"""
    rng = np.random.default_rng(n * 100 + k)
    m, d = 33, 3
    Q, X = grid(rng, m, d), grid(rng, n, d)
    searches = [(Q, X, 0)] + ([(X, X, 1)] if n == m else [])           # (queries, database, same-index flag)
    for A, B, flag in searches:
        Ad, Bd = strided(A, 5, dev), strided(B, 2, dev)
        for metric in ("l2", "dot"):
            want_i, want_v = R.knn(A, B, k, metric, exclude_same=bool(flag))
            one = raw_knn(Ad, Bd, k, metric, flags=flag, splits=1)
            many = raw_knn(Ad, Bd, k, metric, flags=flag, splits=16)
            for got_i, got_v in (one, many):
                assert np.array_equal(got_i, want_i), (metric, flag)
                assert np.array_equal(got_v.astype(np.float64), want_v), (metric, flag)
            assert np.array_equal(one[1].view(np.int32), many[1].view(np.int32)), (metric, flag)
            assert (want_i[:, min(n - flag, k):] == -1).all() and (want_i[:, :min(n - flag, k)] >= 0).all()


# ------------------------------------------------------------------ 6. non-finite values
@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_non_finite_rows_are_never_returned(dev, metric):
    from gae_dgl_amd import ops
    rng = np.random.default_rng(6)
    Q, X = rng.standard_normal((70, 20)).astype(np.float32), rng.standard_normal((400, 20)).astype(np.float32)
    Xb, Qb = X.copy(), Q.copy()
    Xb[3, 0] = NAN; Xb[64, 19] = INF; Xb[65, 7] = -INF; Xb[399, 10] = NAN
    Qb[33, 5] = NAN
    res = ops.knn(torch.from_numpy(Qb).to(dev), torch.from_numpy(Xb).to(dev), k=64, metric=metric)
    idx, val = as_np(res.index), as_np(res.value)
    assert not np.isin(idx, [3, 64, 65, 399]).any()
    pad = INF if metric == "l2" else -INF
    assert (idx[33] == -1).all() and (val[33] == pad).all()
    # the other rows: what the search without the bad rows gives, with the indices mapped back
    keep = np.setdiff1d(np.arange(400), [3, 64, 65, 399])
    clean = ops.knn(torch.from_numpy(Q).to(dev), torch.from_numpy(X[keep]).to(dev), k=64, metric=metric)
    others = np.arange(70) != 33
    assert np.array_equal(idx[others], keep[as_np(clean.index)][others])
    assert np.array_equal(val[others], as_np(clean.value)[others])
    want_i, _ = R.knn(Qb, Xb, 64, metric)
    assert np.array_equal(idx == -1, want_i == -1)


def test_fewer_finite_rows_than_k_pad_the_tail(dev):
    from gae_dgl_amd import ops
    X = torch.randn(40, 8, device=dev)
    X[5:] = NAN
    res = ops.knn(X, k=8)
    idx = as_np(res.index)
    assert (idx[:5, :4] >= 0).all() and (idx[:5, 4:] == -1).all() and (idx[5:] == -1).all()
    assert bool((res.value[:5, 4:] == INF).all())


# ------------------------------------------------------------------ 7. beyond the dense route
def test_two_hundred_thousand_rows(dev):
    from gae_dgl_amd import ops
    n, d, k = 200000, 16, 8
    g = torch.Generator(device="cpu").manual_seed(7)
    X = torch.randn(n, d, generator=g)
    res = ops.knn(X.to(dev), k=k)
    idx, val = as_np(res.index), as_np(res.value)
    assert idx.min() >= 0 and idx.max() < n and not (idx == np.arange(n)[:, None]).any()
    assert (np.diff(val, axis=1) >= 0).all() and np.isfinite(val).all()
    rows = np.random.default_rng(7).choice(n, 256, replace=False)
    rows[:4] = [0, 31, n - 33, n - 1]
    bad = R.check_tolerant(X.numpy(), X.numpy(), idx[rows], val[rows], exclude_same=True, rows=rows)
    assert bad == [], bad[:5]


# ------------------------------------------------------------------ 8. end to end
def fresh_graph(g, dev):
    import gae_dgl_amd as G
    gr = G.DGLGraph()
    gr.add_nodes(int(g["n"]))
    gr.add_edges(g["src"], g["dst"])
    gr.to(dev)
    gr.ndata['h'] = torch.from_numpy(g["X"]).to(dev)
    return gr


def test_nearest_graphs_is_knn_of_the_molecule_features(dev):
    import gae_dgl_amd as G
    from gae_dgl_amd import ops
    from gae_dgl_amd.dataset import DeviceGraphDataset
    data = DeviceGraphDataset.synthetic_zinc(2000, seed=1, device=dev)
    torch.manual_seed(0)
    model = G.GAE(39, [32, 16]).to(dev).eval()
    feats = model.embed_graphs(data)
    res = model.nearest_graphs(data, 10)
    want = ops.knn(feats, k=10)
    assert torch.equal(res.index, want.index) and torch.equal(res.value, want.value)
    assert R.check_tolerant(as_np(feats), as_np(feats), as_np(res.index), as_np(res.value), exclude_same=True) == []
    # queries against the set: a graph that is in both is its own nearest neighbour
    q_ids = [7, 1999, 250]
    hit = model.nearest_graphs(data, 3, queries=data.subset(q_ids), metric="cosine")
    assert as_np(hit.index)[:, 0].tolist() == q_ids and as_np(hit.value)[:, 0] == pytest.approx(1.0, abs=1e-6)
    want = ops.knn(feats[q_ids], feats, k=3, metric="cosine")
    assert torch.equal(hit.index, want.index) and torch.equal(hit.value, want.value)
    # a subset in which some molecules appear twice: each twin lists the other first, at distance 0.0
    ids = np.array([3, 10, 500, 3, 77, 500, 1200], dtype=np.int64)
    twins = model.nearest_graphs(data.subset(ids), 2)
    ti, tv = as_np(twins.index), as_np(twins.value)
    for a, b in ((0, 3), (3, 0), (2, 5), (5, 2)):
        assert ti[a, 0] == b and tv[a, 0] == 0.0
    with pytest.raises(ValueError):
        model.nearest_graphs(data, 3, grad=True)


def test_nearest_nodes_of_gae_and_vgae(dev):
    import gae_dgl_amd as G
    from gae_dgl_amd.vgae import VGAE
    g = load_golden("sym200")
    model = G.GAE(g["X"].shape[1], [int(h) for h in g["hidden"]])
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd/")})
    model = model.to(dev)
    gr = fresh_graph(g, dev)
    feat = gr.ndata['h']
    res = model.nearest_nodes(gr, 6)
    assert gr.ndata['h'] is feat
    with torch.no_grad():
        Z = as_np(model.encode(fresh_graph(g, dev)))
    assert res.index.shape == (Z.shape[0], 6)
    assert R.check_tolerant(Z, Z, as_np(res.index), as_np(res.value), exclude_same=True) == []
    torch.manual_seed(0)
    vg = VGAE(g["X"].shape[1], [32, 16]).to(dev)
    gr = fresh_graph(g, dev)
    feat = gr.ndata['h']
    res = vg.nearest_nodes(gr, 6)
    assert gr.ndata['h'] is feat
    with torch.no_grad():
        mu = as_np(vg.encode(fresh_graph(g, dev))[0])
    assert R.check_tolerant(mu, mu, as_np(res.index), as_np(res.value), exclude_same=True) == []


def test_no_fallback_and_argument_errors(dev):
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    X = torch.randn(40, 8, device=dev)
    for bad in (dict(k=0), dict(k=65)):
        with pytest.raises(GaeHipError):
            ops.knn(X, **bad)
    with pytest.raises(GaeHipError):
        ops.knn(torch.randn(40, 257, device=dev), k=3)
    with pytest.raises(GaeHipError):
        ops.knn(X, torch.randn(40, 9, device=dev), k=3)
    with pytest.raises(GaeHipError):
        ops.knn(X.double(), k=3)
    Z = X.clone(); Z[4] = 0
    with pytest.raises(GaeHipError):
        ops.knn(Z, k=3, metric="cosine")


def test_cli_train_transductive_knn(tmp_path, capsys):
    from gae_dgl_amd import metrics
    from gae_dgl_amd import train_transductive as TT
    rng = np.random.default_rng(0)
    n, c = 300, 3
    comm = rng.integers(0, c, n)
    a = rng.integers(0, n, 6000); b = rng.integers(0, n, 6000)
    keep = (comm[a] == comm[b]) & (a != b)
    a, b = a[keep], b[keep]
    feats = np.eye(c, dtype=np.float32)[comm] + 0.1 * rng.standard_normal((n, c)).astype(np.float32)
    classes = comm.copy(); classes[:10] = -1
    os.makedirs(tmp_path / "data", exist_ok=True)
    np.savez(tmp_path / "data" / "cora.npz", src=np.concatenate([a, b]), dst=np.concatenate([b, a]), features=feats, n=n,
             labels=classes)
    argv = ["--dataset", "cora", "--data_root", str(tmp_path / "data"), "-e", "20", "-s", str(tmp_path), "--seed", "0",
            "--log_every", "1000", "--knn", "5"]
    TT.main(argv)
    text = capsys.readouterr().out
    line = [l for l in text.splitlines() if l.startswith("kNN K = 5 (l2, leave-one-out) accuracy:")]
    assert len(line) == 1, text
    last = TT.main.last_knn
    idx, val = as_np(last["result"].index), as_np(last["result"].value)
    # the lists themselves against the embedding of the trained model, re-encoded here
    last["graph"].ndata['h'] = last["features"]
    with torch.no_grad():
        Z = as_np(last["model"].encode(last["graph"]))
    assert idx.shape == (n, 5) and R.check_tolerant(Z, Z, idx, val, exclude_same=True) == []
    # numpy recomputation of the printed figure from the lists: plurality of the labelled neighbours, ties to the lower class
    votes = np.where(idx >= 0, classes[np.maximum(idx, 0)], -1)
    counts = np.stack([(votes == q).sum(1) for q in range(c)], 1)
    pred = np.where(counts.sum(1) > 0, counts.argmax(1), -1)
    scored = (classes >= 0) & (pred >= 0)
    acc = float((pred[scored] == classes[scored]).mean())
    assert float(line[0].split("accuracy:")[1].split("|")[0]) == pytest.approx(acc, abs=1e-4)
    assert f"nodes scored: {int(scored.sum())} of {n}" in line[0] and scored.sum() == n - 10
    assert acc > 0.9                                                   # three clean communities
    # no labels: it says so
    np.savez(tmp_path / "data" / "cora.npz", src=np.concatenate([a, b]), dst=np.concatenate([b, a]), features=feats, n=n)
    TT.main(argv)
    assert "carries no class labels" in capsys.readouterr().out


def test_cli_embed_neighbours(tmp_path, capsys):
    from gae_dgl_amd import embed as E
    import gae_dgl_amd as G
    torch.manual_seed(0)
    ckpt = str(tmp_path / "m.pkl")
    torch.save(G.GAE(39, [32, 16]).state_dict(), ckpt)
    ng, k = 300, 4
    y = np.random.default_rng(1).standard_normal(ng)
    np.save(tmp_path / "y.npy", y)
    E.main(["--checkpoint", ckpt, "--hidden_dims", "32", "16", "--synthetic", str(ng), "--out", str(tmp_path / "f.npy"),
            "--neighbours", str(k), "--neighbours_out", str(tmp_path / "nn.npz"), "--targets", str(tmp_path / "y.npy")])
    text = capsys.readouterr().out
    assert f"Searched {ng} molecules for their {k} nearest (l2)" in text
    line = [l for l in text.splitlines() if l.startswith(f"kNN ({k}, leave-one-out) RMSE:")]
    assert len(line) == 1, text
    z = np.load(tmp_path / "nn.npz")
    feats = np.load(tmp_path / "f.npy")
    assert z["index"].dtype == np.int32 and z["index"].shape == (ng, k) and z["value"].dtype == np.float32
    assert R.check_tolerant(feats, feats, z["index"], z["value"], exclude_same=True) == []
    pred = y[z["index"]].mean(1)
    err = pred - y
    want = {"RMSE": np.sqrt((err ** 2).mean()), "MAE": np.abs(err).mean(),
            "R2": 1 - (err ** 2).sum() / ((y - y.mean()) ** 2).sum()}
    fields = dict(f.split(":") for f in line[0].split("leave-one-out) ")[1].split(" | "))
    for key, v in want.items():
        assert float(fields[key]) == pytest.approx(v, abs=2e-6)
