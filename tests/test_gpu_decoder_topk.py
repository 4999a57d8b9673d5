"""K16 on the MI355X: gae_decoder_topk / ops.decoder_topk / GAE.predict_links against an fp64 brute force, the
reference's own logits (logits_p0 of the goldens) and exact integer cases where every score and tie is exact."""
import numpy as np
import pytest
import torch

from conftest import CASES, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------ fp64 brute force
def allowed_mask(n, windows=None, csr=None, exclude_self=True):
    """bool [n, n]: the candidates of every row (windows: [n, 2] member windows; csr: host (indptr, indices))"""
    ok = np.ones((n, n), dtype=bool)
    if windows is not None:
        j = np.arange(n)[None, :]
        ok &= (j >= windows[:, :1]) & (j < windows[:, 1:])
    if exclude_self:
        ok[np.arange(n), np.arange(n)] = False
    if csr is not None:
        indptr, indices = csr
        rows = np.repeat(np.arange(n), np.diff(indptr))
        ok[rows, indices] = False
    return ok


def oracle_topk(S, ok, k):
    """exact top-k of S [n, n] (fp64) over the allowed pairs: score descending, j ascending; -1 / -inf padding"""
    n = S.shape[1]
    S = np.where(ok & ~np.isnan(S) & (S != -np.inf), S, -np.inf)
    J = np.broadcast_to(np.arange(n), S.shape)
    r = S.shape[0]
    order = np.lexsort((J, -S), axis=1)[:, :k]
    sc = np.take_along_axis(S, order, 1)
    idx = np.where(np.isfinite(sc) | (sc == np.inf), order, -1)
    sc = np.where(idx >= 0, sc, -np.inf)
    if k > n:
        idx = np.concatenate([idx, np.full((r, k - n), -1)], 1)
        sc = np.concatenate([sc, np.full((r, k - n), -np.inf)], 1)
    return sc, idx


def check_topk(score, index, S, ok, k, tol):
    """(score, index) is A valid top-k of S over ok: allowed indices, scores within tol of S, padding only after the
    candidates run out, and no left-out candidate beats the k-th returned score by more than tol"""
    score = score.cpu().numpy().astype(np.float64); index = index.cpu().numpy()
    n = S.shape[0]
    assert score.shape == (n, k) and index.shape == (n, k)
    n_ok = (ok & np.isfinite(S)).sum(1)
    for i in range(n):
        m = min(k, int(n_ok[i]))
        got = index[i, :m]
        assert (got >= 0).all() and ok[i, got].all(), (i, got)
        assert len(set(got.tolist())) == m
        assert (index[i, m:] == -1).all() and (score[i, m:] == -np.inf).all(), i
        ref = S[i, got]
        scale = np.maximum(1.0, np.abs(ref))
        assert (np.abs(score[i, :m] - ref) <= tol * scale).all(), (i, score[i, :m], ref)
        assert (np.diff(score[i, :m]) <= 0).all(), i
        if m:
            rest = ok[i].copy(); rest[got] = False
            left = S[i, rest]
            left = left[np.isfinite(left)]
            if left.size:
                assert left.max() <= score[i, m - 1] + tol * max(1.0, abs(score[i, m - 1])), i


def as_np(t):
    return t.detach().cpu().numpy()


def host_csr(g):
    indptr, indices = g.csr()
    return as_np(indptr).astype(np.int64), as_np(indices).astype(np.int64)


def build_model(g, dev):
    import gae_dgl_amd as G
    model = G.GAE(g["X"].shape[1], [int(h) for h in g["hidden"]])
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd/")})
    return model.to(dev)


def fresh_graph(g, dev):
    import gae_dgl_amd as G
    gr = G.DGLGraph()
    gr.add_nodes(int(g["n"]))
    gr.add_edges(g["src"], g["dst"])
    gr.to(dev)
    gr.ndata['h'] = torch.from_numpy(g["X"]).to(dev)
    return gr


# ------------------------------------------------------------------ the reference's fixtures
@pytest.mark.parametrize("k", [1, 5, 64])
@pytest.mark.parametrize("case", CASES)
def test_predict_links_matches_reference_logits(case, k, dev):
    g = load_golden(case)
    model = build_model(g, dev)
    gr = fresh_graph(g, dev)
    score, index = model.predict_links(gr, k)
    n = int(g["n"])
    ok = allowed_mask(n, csr=host_csr(gr))
    # the returned scores match the reference's logits at the returned indices (check_topk: to 1e-5), and the set is a
    # top-k of the reference's logits under the exclusions
    check_topk(score, index, g["logits_p0"].astype(np.float64), ok, k, 1e-5)


def _mol8_batch(dev):
    import gae_dgl_amd as G
    parts = load_golden("mol8_parts")
    gs = []
    for i in range(int(parts["n_graphs"])):
        gr = G.DGLGraph()
        gr.add_nodes(int(parts[f"g{i}/n"])); gr.add_edges(parts[f"g{i}/src"], parts[f"g{i}/dst"])
        gr.ndata['h'] = torch.from_numpy(parts[f"g{i}/X"])
        gs.append(gr.to(dev))
    return G.batch(gs)


@pytest.mark.parametrize("k", [1, 5, 64])
def test_mol8_graph_scope_matches_reference_blocks(k, dev):
    whole = load_golden("mol8")
    bg = _mol8_batch(dev)
    model = build_model(whole, dev)
    gp = as_np(bg.graph_ptr())
    n = int(whole["n"])
    member = np.searchsorted(gp, np.arange(n), side="right") - 1
    windows = np.stack([gp[member], gp[member + 1]], 1)
    csr = host_csr(bg)
    X = bg.ndata['h']
    score, index = model.predict_links(bg, k, scope="graph")
    check_topk(score, index, whole["logits_p0"].astype(np.float64), allowed_mask(n, windows, csr), k, 1e-5)
    bg.ndata['h'] = X                                                 # (encode() consumes it, as in gae.py)
    score_b, index_b = model.predict_links(bg, k)                    # batch scope: candidates across molecules too
    check_topk(score_b, index_b, whole["logits_p0"].astype(np.float64), allowed_mask(n, csr=csr), k, 1e-5)


def test_vgae_predict_links_ranks_mu(dev):
    """VGAE.predict_links scores the mean mu (no noise): a top-k of mu mu^T in fp64, not of a sampled z"""
    from gae_dgl_amd.vgae import VGAE
    g = load_golden("sym200")
    torch.manual_seed(0)
    model = VGAE(g["X"].shape[1], [32, 16]).to(dev)
    gr = fresh_graph(g, dev)
    mu, _ = model.encode(gr)
    M = as_np(mu).astype(np.float64)
    gr = fresh_graph(g, dev)
    score, index = model.predict_links(gr, 10)
    n = int(g["n"])
    ok = allowed_mask(n, csr=host_csr(gr))
    check_topk(score, index, M @ M.T, ok, 10, 1e-5)
    gr = fresh_graph(g, dev)
    score2, index2 = model.predict_links(gr, 10)              # no noise drawn: the same answer again
    assert torch.equal(score, score2) and torch.equal(index, index2)


def test_encode_side_effects_unchanged(dev):
    g = load_golden("sym200")
    model = build_model(g, dev)
    a, b = fresh_graph(g, dev), fresh_graph(g, dev)
    model.encode(a)
    model.predict_links(b, 5)
    assert set(a.ndata) == set(b.ndata)
    for key in a.ndata:
        assert torch.equal(a.ndata[key], b.ndata[key])


# ------------------------------------------------------------------ exact integer cases: bit for bit


def _random_csr(rng, n, deg_max, hubs=(), full_rows=()):
    rows = []
    for i in range(n):
        if i in full_rows:
            r = np.arange(n)
        elif i in hubs:
            r = rng.choice(n, size=min(170, n), replace=False)
        else:
            r = rng.integers(0, n, rng.integers(0, deg_max + 1))
        if r.size > 1:
            r = np.concatenate([r, r[:2]])               # repeats
        rng.shuffle(r)                                    # any order
        rows.append(r)
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([r.size for r in rows])
    indices = np.concatenate(rows) if n else np.zeros(0, np.int64)
    return indptr, indices.astype(np.int64)


def _exact_case(n, d, k, dev, seed, ld_pad=3, exclude_self=True, with_edges=True, windows=None, node_ptr=None,
                hubs=(), full_rows=()):
    from gae_dgl_amd import ops
    rng = np.random.default_rng(seed)
    Zi = rng.integers(-2, 3, (n, d)).astype(np.float32)
    if n > 4:
        Zi[n // 2] = Zi[1]                                # equal rows: ties everywhere
    buf = torch.zeros(n, d + ld_pad, dtype=torch.float32, device=dev)
    buf[:, :d] = torch.from_numpy(Zi)
    Z = buf[:, :d]                                        # strided: ldz > d
    csr = _random_csr(rng, n, 6, hubs, full_rows) if with_edges else None
    dcsr = None
    if csr is not None:
        dcsr = (torch.as_tensor(csr[0], dtype=torch.int32, device=dev),
                torch.as_tensor(csr[1], dtype=torch.int32, device=dev))
    score, index = ops.decoder_topk_raw(Z, k, node_ptr, int(np.diff(as_np(node_ptr)).max(initial=0))
                                        if node_ptr is not None else 0, dcsr, exclude_self=exclude_self)
    Z64 = Zi.astype(np.float64)
    ok = allowed_mask(n, windows, csr, exclude_self)
    sc, idx = oracle_topk(Z64 @ Z64.T, ok, k)
    assert np.array_equal(as_np(index), idx)
    assert np.array_equal(as_np(score), sc.astype(np.float32))
    return score, index


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130, 2708])
@pytest.mark.parametrize("d", [1, 3, 16, 17, 64, 256])
def test_exact_integer_case_bit_for_bit(n, d, dev):
    for k in (1, 7, 64):
        _exact_case(n, d, k, dev, seed=n * 1000 + d + k)


def test_exclusions(dev):
    n = 300
    # hub rows of 170 neighbours, rows whose whole window is excluded, shuffled / repeated CSR rows
    _exact_case(n, 16, 10, dev, seed=1, hubs=(3, 77, 150), full_rows=(5, 299))
    _exact_case(n, 16, 64, dev, seed=2, hubs=(3, 77, 150), full_rows=(5, 299))
    _exact_case(n, 16, 10, dev, seed=3, exclude_self=False, hubs=(4,), full_rows=(9,))
    _exact_case(n, 16, 10, dev, seed=4, exclude_self=False, with_edges=False)
    _exact_case(n, 5, 64, dev, seed=5, with_edges=False)


def test_graph_scope_windows(dev, tuning):
    """a batch with empty members, 1-node members and a 20 000-node member; k > most members"""
    sizes = [0, 1, 7, 0, 1, 20000, 3, 0, 1, 40, 1]
    gp = np.zeros(len(sizes) + 1, dtype=np.int64)
    gp[1:] = np.cumsum(sizes)
    n = int(gp[-1])
    member = np.searchsorted(gp, np.arange(n), side="right") - 1
    windows = np.stack([gp[member], gp[member + 1]], 1)
    node_ptr = torch.as_tensor(gp, device=dev)
    rng = np.random.default_rng(0)
    d, k = 16, 10
    Zi = rng.integers(-2, 3, (n, d)).astype(np.float32)
    from gae_dgl_amd import ops
    Z = torch.from_numpy(Zi).to(dev)
    Z64 = Zi.astype(np.float64)
    pick = np.random.default_rng(1)
    for splits in (0, 1, 5):
        tuning("topk_splits", splits)
        score, index = ops.decoder_topk_raw(Z, k, node_ptr, max(sizes), None)
        score, index = as_np(score), as_np(index)
        for g in range(len(sizes)):
            a, b = gp[g], gp[g + 1]
            if a == b:
                continue
            rows = np.arange(a, b)
            if b - a > 500:                               # the 20 000-node member: sampled rows and both ends
                rows = np.unique(np.concatenate([rows[:40], rows[-40:], pick.choice(rows, 200, replace=False)]))
            S = Z64[rows] @ Z64[a:b].T
            ok = np.ones(S.shape, dtype=bool)
            ok[np.arange(len(rows)), rows - a] = False
            sc, idx = oracle_topk(S, ok, k)
            idx = np.where(idx >= 0, idx + a, -1)
            assert np.array_equal(index[rows], idx), (splits, g)
            assert np.array_equal(score[rows], sc.astype(np.float32)), (splits, g)


def test_short_lists_merge_the_same_for_any_split(dev, tuning):
    """the merge of the lane halves and of the column splits (topk_heap.h) on lists shorter than k: members of 1, 5 and
    64 nodes give rows of 0, 4 and 63 candidates at k = 64; n = 70 is two full tiles and a tail of 6.  Integer scores,
    so every split count must give the oracle's bits, padding included"""
    from gae_dgl_amd import ops
    sizes = [1, 5, 64]
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n, d, k = int(gp[-1]), 3, 64
    member = np.searchsorted(gp, np.arange(n), side="right") - 1
    windows = np.stack([gp[member], gp[member + 1]], 1)
    Zi = np.random.default_rng(70).integers(-2, 3, (n, d)).astype(np.float32)
    Z64 = Zi.astype(np.float64)
    sc, idx = oracle_topk(Z64 @ Z64.T, allowed_mask(n, windows), k)
    # the oracle alone: 0, 4 and 63 candidates per row, then -1 / -inf
    n_cand = np.repeat(np.array(sizes) - 1, sizes)
    filled = np.arange(k)[None, :] < n_cand[:, None]
    assert ((idx >= 0) == filled).all() and (idx[~filled] == -1).all() and (sc[~filled] == -np.inf).all()
    Z, node_ptr = torch.from_numpy(Zi).to(dev), torch.as_tensor(gp, device=dev)
    for splits in (1, 3, 16):
        tuning("topk_splits", splits)
        score, index = ops.decoder_topk_raw(Z, k, node_ptr, max(sizes), None)
        assert np.array_equal(as_np(index), idx), splits
        assert np.array_equal(as_np(score), sc.astype(np.float32)), splits


def test_more_splits_than_tiles(dev, tuning):
    """n = 33 is two tiles: with 16 column splits forced, 14 of every panel's parts are empty and their waves write lists
    of padding alone.  Integer scores, so both calls must give the oracle's bits"""
    runs = []
    for splits in (1, 16):
        tuning("topk_splits", splits)
        runs.append(_exact_case(33, 3, 5, dev, seed=33))
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))


def test_single_member_graph_scope_equals_batch_scope(dev):
    import gae_dgl_amd as G
    g = load_golden("sym200")
    model = build_model(g, dev)
    gr = fresh_graph(g, dev)
    s1, i1 = model.predict_links(gr, 10, scope="graph")
    gr = fresh_graph(g, dev)
    s2, i2 = model.predict_links(gr, 10)
    assert torch.equal(i1, i2) and torch.equal(s1, s2)


# ------------------------------------------------------------------ random fp32 at scale
def _tol_check_rows(Z, score, index, rows, k, exclude_self=True):
    """fp64 check of the given rows: 1e-6 |z_i| |z_j| per score, a valid top-k with that tolerance"""
    Zd = Z.double()
    norms = Zd.norm(dim=1)
    for r0 in range(0, len(rows), 64):
        rr = torch.as_tensor(rows[r0:r0 + 64], device=Z.device)
        S = Zd[rr] @ Zd.T
        if exclude_self:
            S[torch.arange(len(rr)), rr] = -np.inf
        bound = 1e-6 * norms[rr, None] * norms[None, :]
        idx = index[rr]
        got = torch.gather(S, 1, idx)
        gb = torch.gather(bound, 1, idx)
        assert (idx >= 0).all()
        assert ((score[rr].double() - got).abs() <= gb).all()
        kth = score[rr, k - 1].double()
        S.scatter_(1, idx, -np.inf)
        assert (S.max(1).values <= kth[:] + 2 * bound.max(1).values).all()


def test_random_pubmed_size(dev):
    from gae_dgl_amd import ops
    torch.manual_seed(0)
    n, d, k = 19717, 16, 10
    Z = torch.randn(n, d, device=dev)
    score, index = ops.decoder_topk(Z, k)
    assert (torch.diff(score, dim=1) <= 0).all()
    _tol_check_rows(Z, score, index, np.random.default_rng(0).choice(n, 1024, replace=False).tolist(), k)


def test_random_200k_rows_beyond_dense(dev):
    from gae_dgl_amd import ops
    torch.manual_seed(1)
    n, d, k = 200_000, 16, 10
    Z = torch.randn(n, d, device=dev)
    score, index = ops.decoder_topk(Z, k)
    assert score.shape == (n, k) and index.shape == (n, k)
    _tol_check_rows(Z, score, index, np.random.default_rng(1).choice(n, 512, replace=False).tolist(), k)


def test_repeatable_and_schedule_independent(dev, tuning):
    from gae_dgl_amd import ops
    torch.manual_seed(2)
    n, d = 2708, 16
    Z = torch.randn(n, d, device=dev)
    Z[100] = Z[7]                                   # equal rows: bit-equal scores, ties resolved by j
    ref = None
    for splits in (0, 1, 2, 7, 16):
        tuning("topk_splits", splits)
        for _ in range(2):
            s, i = ops.decoder_topk(Z, 64)
            if ref is None:
                ref = (s, i)
            assert torch.equal(s, ref[0]) and torch.equal(i, ref[1]), splits
    # equal rows of Z have bit-equal scores: with the same candidates they get the same list
    s, i = ops.decoder_topk(Z, 64, exclude_self=False)
    assert torch.equal(s[7], s[100]) and torch.equal(i[7], i[100])


def test_nan_never_returned(dev):
    from gae_dgl_amd import ops
    torch.manual_seed(3)
    n, d, k = 500, 16, 10
    Z = torch.randn(n, d, device=dev)
    Z[11, 3] = float("nan")
    Z[12, 0] = float("-inf")
    Z[12, 1:] = 0
    score, index = ops.decoder_topk(Z, k)
    torch.cuda.synchronize()
    assert not torch.isnan(score).any()
    assert not (index == 11).any()                  # every score with row 11 is NaN
    assert (index[11] == -1).all() and (score[11] == -np.inf).all()
    assert not ((score == -np.inf) & (index >= 0)).any()      # -inf is never returned as a candidate


# ------------------------------------------------------------------ CLI
def test_cli_recall_and_topk_out(tmp_path, capsys):
    from gae_dgl_amd import train_transductive as TT
    out = tmp_path / "top.npz"
    TT.main(["--dataset", "cora", "-e", "20", "-s", str(tmp_path), "--seed", "0", "--log_every", "100", "--eval",
             "--topk", "10", "--topk_out", str(out)])
    text = capsys.readouterr().out
    line = [l for l in text.splitlines() if l.startswith("test recall@10:")]
    assert line, text
    r = float(line[0].split(":")[1])
    assert 0.0 <= r <= 1.0 and r == pytest.approx(TT.main.last_recall, abs=1e-4)
    z = np.load(out)
    n = 2708
    assert z["index"].shape == (n, 10) and z["index"].dtype == np.int64
    assert z["score"].shape == (n, 10) and z["score"].dtype == np.float32
    # without --topk the output is as before: no recall line
    TT.main(["--dataset", "cora", "-e", "2", "-s", str(tmp_path), "--seed", "0", "--log_every", "100"])
    assert "recall@" not in capsys.readouterr().out
