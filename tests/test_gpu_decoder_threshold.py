"""K22 on the MI355X: gae_decoder_threshold_count / _fill, ops.decoder_threshold and GAE.reconstruct against the dense
fp64 brute force of tests/threshold_ref.py -- bit for bit where fp32 is exact --, against gae_decoder_topk, whose pairs
and score bits it must list, and against the reference's recorded logits."""
import numpy as np
import pytest
import torch

from conftest import CASES, load_golden
from threshold_ref import dense_mask, threshold_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def as_np(t):
    return t.detach().cpu().numpy()


def dev_csr(csr, dev):
    return (torch.as_tensor(csr[0], dtype=torch.int32, device=dev), torch.as_tensor(csr[1], dtype=torch.int32, device=dev))


def same_scores(a, b):
    """fp32 arrays equal bit for bit up to the sign of zero"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all(a == b))


def assert_equal_ref(got, ref, what=""):
    indptr, index, score = got[:3]
    assert indptr.dtype == torch.int64 and index.dtype == torch.int32 and score.dtype == torch.float32, what
    assert np.array_equal(as_np(indptr), ref[0]), what
    assert np.array_equal(as_np(index), ref[1]), what
    assert same_scores(as_np(score), ref[2].astype(np.float32)), what


def _members(n):
    """ragged members of 1..40 nodes, one of them empty, that add up to n: (node_ptr, windows [n, 2])"""
    sizes = {1: [1, 0], 31: [5, 0, 26], 33: [1, 0, 32], 174: [1, 40, 0, 33, 32, 31, 17, 20]}.get(n)
    if sizes is None:
        sizes = [n // 3, 0, n - n // 3]
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert gp[-1] == n
    member = np.searchsorted(gp, np.arange(n), side="right") - 1
    return gp, np.stack([gp[member], gp[member + 1]], 1)


def _random_csr(rng, n, deg_max=6, windows=None):
    """rows in any order with repeated entries; inside the row's window when there is one"""
    rows = []
    for i in range(n):
        lo, hi = (0, n) if windows is None else windows[i]
        r = rng.integers(lo, hi, rng.integers(0, deg_max + 1))
        if r.size > 1:
            r = np.concatenate([r, r[:2]])                # repeated entries
        rng.shuffle(r)                                    # any order
        rows.append(r)
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([r.size for r in rows])
    return indptr, (np.concatenate(rows) if n else np.zeros(0)).astype(np.int64)


def _eighths(rng, n, d):
    """entries that are multiples of 1/8 in [-4, 4]: every product is a multiple of 1/64 and every partial sum of up
    to 256 of them stays below 2^24 / 64, so the fp32 chain is exact and equals the fp64 product"""
    Z = rng.integers(-32, 33, (n, d)).astype(np.float32) / 8
    if n > 4:
        Z[n // 2] = Z[1]                                  # equal rows: ties everywhere
    return Z


def _strided(Zi, dev, pad=3):
    buf = torch.zeros(Zi.shape[0], Zi.shape[1] + pad, dtype=torch.float32, device=dev)
    buf[:, :Zi.shape[1]] = torch.from_numpy(Zi)
    return buf[:, :Zi.shape[1]]                           # ldz > d


def _attained(Zi, q):
    """a threshold some pair attains: the q-quantile element of Z Z^T"""
    S = np.sort((Zi.astype(np.float64) @ Zi.astype(np.float64).T).reshape(-1))
    return float(S[min(int(q * S.size), S.size - 1)])


# ------------------------------------------------------------------ exact cases: bit for bit
@pytest.mark.parametrize("n", [1, 31, 33, 174])
@pytest.mark.parametrize("d", [16, 20, 64, 130])
def test_exact_case_bit_for_bit(n, d, dev):
    """every <DH, ONE> form and a feature tail (d = 20, 130), one panel and several, members that start and end off the
    tile boundaries, 1 and 3 column splits, both scopes, the four flag combinations; thresholds that are attained"""
    from gae_dgl_amd import ops
    rng = np.random.default_rng(n * 1000 + d)
    Zi = _eighths(rng, n, d)
    Z = _strided(Zi, dev)
    gp, windows = _members(n)
    node_ptr = torch.as_tensor(gp, device=dev)
    bound = int(np.diff(gp).max())
    csr = _random_csr(rng, n)
    dcsr = dev_csr(csr, dev)
    thr = _attained(Zi, 0.6)
    S = Zi.astype(np.float64) @ Zi.astype(np.float64).T
    assert (S == thr).any()
    listed = 0
    for wins, scope in ((None, None), (windows, node_ptr)):
        for ex in (True, False):
            for edges in (True, False):
                ref = threshold_ref(Zi, thr, wins, csr if edges else None, ex)
                listed += ref[1].size
                for splits in (1, 3):
                    got = ops.decoder_threshold_raw(Z, thr, scope, bound, dcsr if edges else None, exclude_self=ex,
                                                    splits=splits)
                    assert got[3] == ref[0][-1]
                    assert_equal_ref(got, ref, (n, d, scope is not None, ex, edges, splits))
    assert listed > 0 or n == 1
    # a threshold nothing reaches, and one everything reaches
    top = float(S.max())
    got = ops.decoder_threshold_raw(Z, np.nextafter(np.float32(top), np.float32(np.inf)), None, 0, None, exclude_self=False)
    assert got[3] == 0 and as_np(got[0]).tolist() == [0] * (n + 1) and got[1].numel() == 0
    assert_equal_ref(ops.decoder_threshold_raw(Z, top, None, 0, None, exclude_self=False),
                     threshold_ref(Zi, top, None, None, False))
    assert_equal_ref(ops.decoder_threshold_raw(Z, float("-inf"), node_ptr, bound, dcsr, splits=3),
                     threshold_ref(Zi, float("-inf"), windows, csr, True))


def test_empty_embedding(dev):
    from gae_dgl_amd import ops
    got = ops.decoder_threshold_raw(torch.zeros(0, 16, device=dev), 0.0)
    assert as_np(got[0]).tolist() == [0] and got[1].numel() == 0 and got[2].numel() == 0 and got[3] == 0


# ------------------------------------------------------------------ every column split writes the same bytes
@pytest.mark.parametrize("n", [174, 1000])
def test_split_independent(n, dev):
    from gae_dgl_amd import ops
    torch.manual_seed(n)
    rng = np.random.default_rng(n)
    Z = torch.randn(n, 16, device=dev)
    Z[n // 2] = Z[7]
    gp, windows = _members(n)
    node_ptr = torch.as_tensor(gp, device=dev)
    dcsr = dev_csr(_random_csr(rng, n), dev)
    for scope in (None, node_ptr):
        ref = None
        for splits in (1, 2, 3, 16, 0):
            got = ops.decoder_threshold_raw(Z, 0.25, scope, int(np.diff(gp).max()), dcsr, splits=splits)
            if ref is None:
                ref = got
                assert got[3] > n
                continue
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), (n, splits)
            assert torch.equal(got[2].view(torch.int32), ref[2].view(torch.int32)), (n, splits)


# ------------------------------------------------------------------ the pairs and the bits K16 lists
@pytest.mark.parametrize("d", [16, 64])
def test_same_pairs_and_bits_as_topk(d, dev):
    """tau = the 0.98 quantile of the scores of the row of median norm: on the fp64 brute force more than 90 % of the
    rows list at most 64 pairs (95 % at d = 16, all at d = 64).  Each such row, sorted by (score descending, j
    ascending), is the part of gae_decoder_topk's list of 64 at or above tau, scores compared as bits."""
    import gae_dgl_amd as G
    from gae_dgl_amd import ops
    n, k, deg = 1000, 64, 5
    torch.manual_seed(100 + d)
    Zc = torch.randn(n, d)
    gen = torch.Generator(device="cpu").manual_seed(1)
    g = G.DGLGraph((torch.randint(0, n, (deg * n,), generator=gen), torch.arange(n).repeat_interleave(deg)),
                   num_nodes=n).to(dev)                   # every node has 5 in-edges: CSR rows of 5
    indptr, indices = (as_np(t).astype(np.int64) for t in g.csr())
    Z64 = Zc.double().numpy()
    r = int(np.argsort(np.linalg.norm(Z64, axis=1))[n // 2])
    tau = float(np.float32(np.quantile(np.delete(Z64 @ Z64[r], r), 0.98)))
    brute = threshold_ref(Z64, tau, None, (indptr, indices), True)
    assert float((np.diff(brute[0]) <= k).mean()) >= 0.9
    Z = Zc.to(dev)
    links = ops.decoder_threshold(Z, tau, g, exclude_edges=True)
    score, index = ops.decoder_topk(Z, k, g)
    ip, ix, sc = as_np(links.indptr), as_np(links.index).astype(np.int64), as_np(links.score)
    tsc, tix = as_np(score), as_np(index)
    counts = np.diff(ip)
    qualify = counts <= k
    assert float(qualify.mean()) >= 0.9
    for i in np.flatnonzero(qualify):
        cols, vals = ix[ip[i]:ip[i + 1]], sc[ip[i]:ip[i + 1]]
        assert (np.diff(cols) > 0).all()
        order = np.lexsort((cols, -vals.astype(np.float64)))
        keep = (tix[i] >= 0) & (tsc[i] >= np.float32(tau))
        assert np.array_equal(cols[order], tix[i][keep]), i
        assert np.array_equal(vals[order].view(np.int32), tsc[i][keep].view(np.int32)), i
    for i in np.flatnonzero(~qualify)[:20]:               # the longer rows hold K16's whole list
        assert set(tix[i].tolist()) <= set(ix[ip[i]:ip[i + 1]].tolist())


# ------------------------------------------------------------------ model level: the reference's recorded logits
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


def _golden_threshold(S):
    """the midpoint of the widest gap among the 400 sorted logits around the 0.99 quantile, and that gap over
    max(1, |tau|)"""
    flat = np.sort(S.reshape(-1))
    k = int(0.99 * flat.size)
    w = flat[max(0, k - 200):max(0, k - 200) + 400]
    gaps = np.diff(w)
    a = int(np.argmax(gaps))
    tau = (w[a] + w[a + 1]) / 2
    return float(tau), float(gaps[a] / max(1.0, abs(tau)))


def _check_golden(links, S, ok, tau, tol=1e-5):
    n = S.shape[0]
    ip, ix, sc = as_np(links.indptr), as_np(links.index).astype(np.int64), as_np(links.score).astype(np.float64)
    want = (S >= tau) & ok
    assert ip[-1] == ix.size == sc.size
    assert np.array_equal(dense_mask(ip, ix, n), want)
    rows = np.repeat(np.arange(n), np.diff(ip))
    assert (np.diff(ix)[np.diff(rows) == 0] > 0).all()    # columns ascend within a row
    s = S[rows, ix]
    assert (np.abs(sc - s) <= tol * np.maximum(1.0, np.abs(s))).all()


@pytest.mark.parametrize("case", CASES)
def test_reconstruct_matches_reference_logits(case, dev):
    """tau sits in a gap of the golden logits at least 2e-4 max(1, |tau|) wide -- ten times the suite's 1e-5 parity
    tolerance on each side --, so no pair may legitimately flip: the decoded set is exactly logits_p0 >= tau"""
    g = load_golden(case)
    assert "logits_p0" in g
    S = g["logits_p0"].astype(np.float64)
    tau, rel_gap = _golden_threshold(S)
    print(f"{case}: tau {tau:.6f}, gap / max(1, |tau|) {rel_gap:.3e}, {int((S >= tau).sum())} pairs")
    assert rel_gap >= 2e-4
    model = build_model(g, dev)
    gr = fresh_graph(g, dev)
    feat = gr.ndata['h']
    links = model.reconstruct(gr, threshold=tau, exclude_self=False)
    assert gr.ndata['h'] is feat                          # restored on exit
    n = int(g["n"])
    _check_golden(links, S, np.ones((n, n), dtype=bool), tau)
    row, col = links.pairs()
    assert row.dtype == col.dtype == torch.int64 and row.numel() == int((S >= tau).sum())
    assert np.array_equal(np.stack([as_np(row), as_np(col)]), np.stack(np.nonzero(S >= tau)))


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


def test_mol8_graph_scope_matches_reference_blocks(dev):
    whole = load_golden("mol8")
    bg = _mol8_batch(dev)
    model = build_model(whole, dev)
    gp = as_np(bg.graph_ptr())
    n = int(whole["n"])
    member = np.searchsorted(gp, np.arange(n), side="right") - 1
    block = member[:, None] == member[None, :]
    S = whole["logits_p0"].astype(np.float64)
    tau, rel_gap = _golden_threshold(S)
    assert rel_gap >= 2e-4
    links = model.reconstruct(bg, threshold=tau, scope="graph", exclude_self=False)
    _check_golden(links, S, block, tau)
    assert 0 < int(links.indptr[-1]) < int((S >= tau).sum())          # pairs across molecules are left out
    # the default prob = 0.5 is the threshold 0; self pairs and known bonds left out on request.  mol8 has logits 4e-5
    # from 0, so the set is pinned only outside the suite's 1e-5 parity tolerance: every pair above it, none below
    links = model.reconstruct(bg, scope="graph", exclude_edges=True)
    ok = block & ~np.eye(n, dtype=bool) & ~(whole["adj"] != 0)
    listed = dense_mask(as_np(links.indptr), as_np(links.index).astype(np.int64), n)
    assert not (listed & ~((S >= -1e-5) & ok)).any() and not (((S >= 1e-5) & ok) & ~listed).any()
    assert bool((links.score >= 0).all()) and 0 < int(links.indptr[-1]) < int(ok.sum())


def test_vgae_reconstruct_decodes_mu(dev):
    from gae_dgl_amd import ops
    from gae_dgl_amd.vgae import VGAE
    g = load_golden("sym200")
    torch.manual_seed(0)
    model = VGAE(g["X"].shape[1], [32, 16]).to(dev)
    gr = fresh_graph(g, dev)
    feat = gr.ndata['h']
    mu, _ = model.encode(fresh_graph(g, dev))
    links = model.reconstruct(gr, prob=0.6)
    assert gr.ndata['h'] is feat
    direct = ops.decoder_threshold(mu.detach().contiguous(), ops.threshold_of_prob(0.6))
    for x, y in zip(links, direct):
        assert torch.equal(x, y)
    assert int(links.indptr[-1]) > 0


# ------------------------------------------------------------------ NaN, infinities
def test_special_values(dev):
    from gae_dgl_amd import ops
    rng = np.random.default_rng(8)
    n, d = 200, 16
    Zi = rng.integers(-2, 3, (n, d)).astype(np.float32)
    Zi[11, 3] = np.nan                                    # every score with node 11 is NaN
    Zi[12, 0] = -np.inf                                   # s_{i,12} = -inf, +inf or NaN with the sign of z_i[0]
    Zi[12, 1:] = 0
    Zi[13, 0] = np.inf
    Zi[13, 1:] = 0
    Z = torch.from_numpy(Zi).to(dev)
    with np.errstate(invalid="ignore"):
        S = Zi.astype(np.float64) @ Zi.astype(np.float64).T
    assert np.isnan(S).any() and (S == np.inf).any() and (S == -np.inf).any()
    for thr in (float("-inf"), float("inf"), 1.0):
        for splits in (1, 2):
            got = ops.decoder_threshold_raw(Z, thr, exclude_self=False, splits=splits)
            ref = threshold_ref(Zi, thr, None, None, False)
            assert_equal_ref(got, ref, thr)
            sc = as_np(got[2])
            assert not np.isnan(sc).any() and not (sc == -np.inf).any()
            if thr == float("-inf"):                      # all candidates: everything but NaN and -inf
                assert got[3] == int((~np.isnan(S) & (S != -np.inf)).sum()) > 0
            if thr == float("inf"):
                assert got[3] == int((S == np.inf).sum()) > 0 and (sc == np.inf).all()
            assert int(got[0][12]) == int(got[0][11])     # the NaN row lists nothing


# ------------------------------------------------------------------ capacity
def test_capacity_guards_every_store(dev):
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    torch.manual_seed(3)
    n = 300
    Z = torch.randn(n, 16, device=dev)
    full = ops.decoder_threshold_raw(Z, 1.0, splits=3)
    total = full[3]
    assert total > 1000
    cap = total - 7
    index = torch.full((total + 64,), -7, dtype=torch.int32, device=dev)
    score = torch.full((total + 64,), -123.0, dtype=torch.float32, device=dev)
    got = ops.decoder_threshold_raw(Z, 1.0, splits=3, capacity=cap, out=(index, score))
    assert got[3] == total and torch.equal(got[0], full[0])
    assert torch.equal(index[:cap], full[1][:cap])
    assert torch.equal(score[:cap].view(torch.int32), full[2][:cap].view(torch.int32))
    assert bool((index[cap:] == -7).all()) and bool((score[cap:] == -123.0).all())       # the canaries are intact
    with pytest.raises(GaeHipError, match=str(total)) as e:
        ops.decoder_threshold(Z, 1.0, max_pairs=total - 1)
    assert "max_pairs" in str(e.value) and "threshold" in str(e.value)
    links = ops.decoder_threshold(Z, 1.0, max_pairs=total)
    assert torch.equal(links.index, full[1]) and torch.equal(links.indptr, full[0])


# ------------------------------------------------------------------ metrics end to end
def test_metrics_of_a_decode_equal_the_dense_ones(dev):
    from gae_dgl_amd import metrics, ops
    n, d = 174, 16
    rng = np.random.default_rng(5)
    Zi = _eighths(rng, n, d)
    gp, windows = _members(n)
    thr = _attained(Zi, 0.8)
    ref = threshold_ref(Zi, thr, windows, None, True)
    P = dense_mask(ref[0], ref[1], n)
    # the truth: the prediction itself on the first four members, random bonds (with repeats) on the others
    rand = _random_csr(rng, n, 6, windows)
    rows = [ref[1][ref[0][i]:ref[0][i + 1]] if i < gp[4] else rand[1][rand[0][i]:rand[0][i + 1]] for i in range(n)]
    true = (np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64), np.concatenate(rows))
    T = dense_mask(true[0], true[1], n) & ~np.eye(n, dtype=bool)
    got = ops.decoder_threshold_raw(_strided(Zi, dev), thr, torch.as_tensor(gp, device=dev), int(np.diff(gp).max()))
    assert_equal_ref(got, ref)
    out = metrics.reconstruction_metrics(got[0], got[1], *dev_csr(true, dev), node_ptr=torch.as_tensor(gp, device=dev))
    tp, fp, fn = int((P & T).sum()), int((P & ~T).sum()), int((~P & T).sum())
    assert (out["tp"], out["fp"], out["fn"], out["n_pred"]) == (tp, fp, fn, int(P.sum()))
    assert tp > 0 and fp > 0 and fn > 0
    assert out["precision"] == pytest.approx(tp / (tp + fp)) and out["recall"] == pytest.approx(tp / (tp + fn))
    assert out["f1"] == pytest.approx(2 * tp / (2 * tp + fp + fn))
    exact = np.array([np.array_equal(P[gp[k]:gp[k + 1]], T[gp[k]:gp[k + 1]]) for k in range(len(gp) - 1)])
    assert exact[:4].all() and not exact.all()
    assert np.array_equal(as_np(out["exact"]), exact) and out["exact_fraction"] == pytest.approx(exact.mean())


# ------------------------------------------------------------------ CLI
def test_cli_decode_out(tmp_path, capsys):
    import os
    import gae_dgl_amd as G
    from gae_dgl_amd import metrics
    from gae_dgl_amd import train_transductive as TT
    rng = np.random.default_rng(0)
    n, k = 300, 5
    comm = rng.integers(0, k, n)
    a = rng.integers(0, n, 6000); b = rng.integers(0, n, 6000)
    keep = (comm[a] == comm[b]) & (a != b)
    a, b = a[keep], b[keep]
    src, dst = np.concatenate([a, b]), np.concatenate([b, a])
    feats = np.eye(k, dtype=np.float32)[comm] + 0.1 * rng.standard_normal((n, k)).astype(np.float32)
    os.makedirs(tmp_path / "data", exist_ok=True)
    np.savez(tmp_path / "data" / "cora.npz", src=src, dst=dst, features=feats, n=n)
    out = tmp_path / "decoded.npz"
    TT.main(["--dataset", "cora", "--data_root", str(tmp_path / "data"), "-e", "20", "-s", str(tmp_path), "--seed", "0",
             "--log_every", "1000", "--decode_out", str(out), "--decode_prob", "0.7"])
    text = capsys.readouterr().out
    line = [l for l in text.splitlines() if l.startswith("reconstruction precision:")]
    assert len(line) == 1, text
    fields = dict(f.rsplit(":", 1) for f in line[0].split(" | "))
    z = np.load(out)
    assert z["indptr"].dtype == np.int64 and z["index"].dtype == np.int32 and z["score"].dtype == np.float32
    assert z["indptr"].shape == (n + 1,) and z["indptr"][-1] == len(z["index"]) == len(z["score"]) > 0
    assert (z["score"] >= np.float32(np.log(0.7 / 0.3))).all()
    g = G.DGLGraph((src, dst), num_nodes=n).to(torch.device("cuda:0"))
    rm = metrics.reconstruction_metrics(z["indptr"], z["index"], *(t.cpu() for t in g.csr()))
    assert rm == {k_: v for k_, v in TT.main.last_decode.items()}
    assert float(fields["reconstruction precision"]) == pytest.approx(rm["precision"], abs=1e-4)
    assert float(fields["recall"]) == pytest.approx(rm["recall"], abs=1e-4)
    assert float(fields["F1"]) == pytest.approx(rm["f1"], abs=1e-4)
    assert int(fields["predicted pairs"]) == rm["n_pred"] == len(z["index"])
    # without the flag the output is as before: no such line, no file
    TT.main(["--dataset", "cora", "--data_root", str(tmp_path / "data"), "-e", "2", "-s", str(tmp_path), "--seed", "0",
             "--log_every", "1000"])
    assert "reconstruction" not in capsys.readouterr().out
