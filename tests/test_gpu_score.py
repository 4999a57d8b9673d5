"""GAE.score_graphs / ops.score_graphs (K20, gae_score_graphs): per-molecule counts behind ROC-AUC, average precision and
the no-dropout loss from one fused launch -- integer-exact against the numpy reference (score_ref) where fp32 is exact,
inside the band the project's tolerance leaves open elsewhere, bit for bit across subsets / positions / repeats / runs,
against K15's per-member loss, through every route and through the scripts."""
import os

import numpy as np
import pytest
import torch

import score_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-5
INTS = ("n_pos", "n_neg", "wins", "ties")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def close(a, b, tol):
    """both NaN, or within tol of max(1, |reference|) (the suite's measure)"""
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= tol * max(1.0, abs(b))


def host(scores):
    return {k: getattr(scores, k).cpu().numpy() for k in scores._fields}


def check_exact(got, ref_rows, what):
    """integer equality, ap within 1e-12 relative, loss within the suite's 1e-5; the figures are printed first"""
    g = host(got)
    worst_ap = worst_loss = 0.0
    for k, r in enumerate(ref_rows):
        if not np.isnan(r["ap"]) and not np.isnan(g["ap"][k]):
            worst_ap = max(worst_ap, abs(g["ap"][k] - r["ap"]) / abs(r["ap"]))
        if not np.isnan(r["loss"]) and not np.isnan(g["loss"][k]):
            worst_loss = max(worst_loss, abs(g["loss"][k] - r["loss"]) / max(1.0, abs(r["loss"])))
    print(f"{what}: {len(ref_rows)} graphs, worst ap error {worst_ap:.3e} (relative), worst loss error {worst_loss:.3e}")
    for k, r in enumerate(ref_rows):
        assert [int(g[f][k]) for f in INTS] == [r[f] for f in INTS], (what, k, [int(g[f][k]) for f in INTS], [r[f] for f in INTS])
        assert (np.isnan(r["ap"]) and np.isnan(g["ap"][k])) or abs(g["ap"][k] - r["ap"]) <= 1e-12 * abs(r["ap"]), (what, k)
        assert close(float(g["loss"][k]), r["loss"], TOL), (what, k, g["loss"][k], r["loss"])
        assert close(g["auc"][k], r["auc"], 1e-15), (what, k)


def to_dev(dev, gp, indptr, indices):
    return (torch.from_numpy(np.asarray(gp, dtype=np.int64)).to(dev), torch.from_numpy(indptr).to(dev),
            torch.from_numpy(indices).to(dev))


def make_ds(gp, rows, cols, X, dev, storage="uint8"):
    from gae_dgl_amd.dataset import DeviceGraphDataset
    return DeviceGraphDataset(gp, cols, rows, X, device=dev, feat_storage=storage)        # (src = column, dst = row)


def make_model(f_in, Ws, bs, norm, dev):
    import gae_dgl_amd as G
    model = G.GAE(f_in, [int(W.shape[0]) for W in Ws], norm=None if norm == "none" else norm)
    with torch.no_grad():
        for layer, W, b in zip(model.layers, Ws, bs):
            layer.apply_mod.linear.weight.copy_(torch.from_numpy(W))
            layer.apply_mod.linear.bias.copy_(torch.from_numpy(b))
    return model.to(dev)


def random_model(hidden, norm, dev, seed=0, f_in=39):
    import gae_dgl_amd as G
    torch.manual_seed(seed)
    model = G.GAE(f_in, hidden, norm=None if norm == "none" else norm)
    with torch.no_grad():
        for l in model.layers:
            l.apply_mod.linear.bias.uniform_(-0.5, 0.5)
    return model.to(dev)


def params_of(model):
    return ([l.apply_mod.linear.weight.detach().cpu().numpy() for l in model.layers],
            [l.apply_mod.linear.bias.detach().cpu().numpy() for l in model.layers])


# ------------------------------------------------------------------ 1. exact, Z given (n_layers = 0)
def _shapes(rng, which):
    """(gp, indptr, indices): the CSR the kernel reads, entries in the order given"""
    if which == "zinc":
        gp, rows, cols = R.molecule_set(rng, rng.integers(6, 39, 300))
    elif which == "directed":
        gp, rows, cols = R.molecule_set(rng, rng.integers(1, 40, 200), directed=True)
    else:
        # graphs of 0, 1, 2 and 64 nodes; edgeless and complete graphs; a self loop alone; entries that point outside
        sizes = [1, 2, 64, 0, 5, 64, 2, 1, 6, 64, 3, 0, 7, 4]
        gp, rows, cols = R.molecule_set(rng, sizes)
        graph_of = np.searchsorted(gp, rows, side="right") - 1
        keep = ~np.isin(graph_of, [4, 5, 6, 9])                       # 4 and 9 (64 nodes) stay edgeless
        rows, cols = list(rows[keep]), list(cols[keep])
        for g, self_loops in ((5, False), (6, True)):                 # complete: 64 nodes; 2 nodes with self loops
            for i in range(gp[g], gp[g + 1]):
                for j in range(gp[g], gp[g + 1]):
                    if i != j or self_loops:
                        rows.append(i); cols.append(j)
        rows += [gp[7]]; cols += [gp[7]]                              # graph 7: one node, a self loop alone
        rows += [gp[12], gp[12] + 1, gp[12] + 1, gp[13]]              # columns outside the row's own graph
        cols += [gp[2], gp[11], gp[14] - 1, gp[1]]
        rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    indptr, indices = R.csr_rows(int(gp[-1]), rows, cols)
    return gp, indptr, indices


@pytest.mark.parametrize("exclude_self", [True, False])
@pytest.mark.parametrize("d", [1, 7, 16, 33, 64])
@pytest.mark.parametrize("which", ["zinc", "directed", "corners"])
def test_given_integer_embedding_is_scored_exactly(which, d, exclude_self, dev):
    from gae_dgl_amd import ops
    rng = np.random.default_rng(100 + d)
    gp, indptr, indices = _shapes(rng, which)
    Z = rng.integers(-8, 9, (int(gp[-1]), d)).astype(np.float32)
    ref = [R.graph_scores(Z, indptr, indices, int(gp[g]), int(gp[g + 1] - gp[g]), exclude_self) for g in range(len(gp) - 1)]
    got = ops.score_graphs(*to_dev(dev, gp, indptr, indices), torch.from_numpy(Z).to(dev), exclude_self=exclude_self)
    check_exact(got, ref, f"Z given, {which}, d={d}, exclude_self={exclude_self}")
    if which == "corners":
        g = host(got)
        assert np.isnan(g["loss"][4]) and np.isnan(g["ap"][4]) and np.isnan(g["auc"][4]) and g["n_pos"][4] == 0     # edgeless
        # complete: graph 6 lists its self loops too, graph 5 does not -- its diagonal is 64 negatives when self pairs count
        assert g["n_neg"][6] == 0 and np.isnan(g["ap"][6]) and np.isnan(g["auc"][6]) and not np.isnan(g["loss"][6])
        assert g["n_neg"][5] == (0 if exclude_self else 64) and np.isnan(g["ap"][5]) == exclude_self and not np.isnan(g["loss"][5])
        assert [int(g[f][3]) for f in INTS] == [0, 0, 0, 0] and np.isnan(g["loss"][3])                               # empty
        assert (g["n_pos"][7] == 0) == exclude_self                                                                  # a self loop alone


def test_refused_graphs_and_non_finite_logits_give_minus_one(dev):
    from gae_dgl_amd import ops
    rng = np.random.default_rng(1)
    gp, rows, cols = R.molecule_set(rng, [5, 70, 6, 7])
    indptr, indices = R.csr_rows(int(gp[-1]), rows, cols)
    Z = rng.integers(-3, 4, (int(gp[-1]), 8)).astype(np.float32)
    Z[gp[2] + 1, 3] = np.inf
    ids = torch.tensor([0, 1, 2, 3, 9, -1, 0], dtype=torch.int64, device=dev)
    got = host(ops.score_graphs(*to_dev(dev, gp, indptr, indices), torch.from_numpy(Z).to(dev), graph_ids=ids,
                                max_graph_nodes=64))
    for k in (1, 2, 4, 5):              # above 64 rows, a non-finite logit, ids outside the set
        assert [int(got[f][k]) for f in INTS] == [-1] * 4 and np.isnan(got["ap"][k]) and np.isnan(got["loss"][k]) \
            and np.isnan(got["auc"][k]), k
    ref = R.graph_scores(Z, indptr, indices, 0, 5)
    for k in (0, 6):
        assert [int(got[f][k]) for f in INTS] == [ref[f] for f in INTS]
    # a bound below a graph's size refuses that graph instead of overrunning the block
    low = host(ops.score_graphs(*to_dev(dev, gp, indptr, indices), torch.from_numpy(Z).to(dev), max_graph_nodes=6))
    assert int(low["n_pos"][3]) == -1 and int(low["n_pos"][0]) == ref["n_pos"]


# ------------------------------------------------------------------ 2. exact, fused encoder
@pytest.mark.parametrize("exclude_self", [True, False])
@pytest.mark.parametrize("hidden", [[8, 4], [16, 8, 4]], ids=lambda h: "x".join(map(str, h)))
def test_integer_encoder_is_scored_exactly(hidden, exclude_self, dev):
    gp, rows, cols, X, Ws, bs = R.integer_fixture(hidden)
    indptr, indices = R.csr_rows(int(gp[-1]), rows, cols)
    ref, _ = R.set_scores(gp, indptr, indices, X, Ws, bs, "none", exclude_self, integers=True)
    model = make_model(39, Ws, bs, "none", dev)
    got = model.score_graphs(make_ds(gp, rows, cols, X, dev), fused=True, exclude_self=exclude_self)
    check_exact(got, ref, f"integer encoder {hidden}, exclude_self={exclude_self}")
    assert int(got.ties.clamp(min=0).sum()) > 1000


# ------------------------------------------------------------------ 3. general weights: the band
def check_band(got, bands, what):
    """lo <= wins and wins + ties <= hi per molecule (score_ref.band: a logit error of at most delta leaves exactly the
    comparisons within 2 delta open); ap between the oracle's AP with every comparison shifted by -2 delta and by
    +2 delta; loss within 1e-5 of fp64.  The figures are printed first."""
    g = host(got)
    slack = max((b["hi"] - b["lo"]) for b in bands)
    used = max(max(b["wins"] - int(g["wins"][k]), int(g["wins"][k] + g["ties"][k]) - b["wins"] - b["ties"], 0)
               for k, b in enumerate(bands))
    worst_loss = max(abs(float(g["loss"][k]) - b["loss"]) / max(1.0, abs(b["loss"])) for k, b in enumerate(bands)
                     if not np.isnan(b["loss"]))
    worst_ap = max(abs(float(g["ap"][k]) - b["ap"]) for k, b in enumerate(bands) if not np.isnan(b["ap"]))
    print(f"{what}: widest band {slack} pairs, largest departure of the counts from the oracle's {used}, "
          f"worst |ap - oracle| {worst_ap:.3e}, worst loss error {worst_loss:.3e}")
    for k, b in enumerate(bands):
        assert (int(g["n_pos"][k]), int(g["n_neg"][k])) == (b["n_pos"], b["n_neg"]), (what, k)
        assert b["lo"] <= int(g["wins"][k]) and int(g["wins"][k] + g["ties"][k]) <= b["hi"], (what, k)
        if not np.isnan(b["ap"]):
            assert b["ap_lo"] - 1e-12 <= float(g["ap"][k]) <= b["ap_hi"] + 1e-12, (what, k)
        assert close(float(g["loss"][k]), b["loss"], TOL), (what, k, g["loss"][k], b["loss"])


@pytest.mark.parametrize("norm", ["none", "both"])
def test_general_weights_stay_inside_the_band(norm, dev):
    gp, rows, cols, X, Ws, bs = R.band_fixture()
    indptr, indices = R.csr_rows(int(gp[-1]), rows, cols)
    _, logits = R.set_scores(gp, indptr, indices, X, Ws, bs, norm)
    bands, delta, open_pairs, pairs = R.band_totals(gp, indptr, indices, logits)
    assert open_pairs <= 0.01 * pairs
    model = make_model(39, Ws, bs, norm, dev)
    got = model.score_graphs(make_ds(gp, rows, cols, X, dev, "float32"), fused=True)
    check_band(got, bands, f"band, norm={norm}, delta={delta:.3e}")


# ------------------------------------------------------------------ 4. the loss is K15's
@pytest.mark.parametrize("norm", ["none", "both"])
def test_loss_is_the_per_member_loss_of_decoder_bce_graphs(norm, dev):
    from gae_dgl_amd import ops
    rng = np.random.default_rng(31)
    sizes = rng.integers(2, 39, 200)
    sizes[[5, 50]] = 1                                   # members without an edge: left out by K15, NaN here
    gp, rows, cols = R.molecule_set(rng, sizes)
    X = (rng.random((int(gp[-1]), 39)) < 0.15).astype(np.float32)
    ds = make_ds(gp, rows, cols, X, dev)
    model = random_model([32, 16], norm, dev, seed=2)
    bg = ds.batch(np.arange(len(sizes)))
    if norm == "both":
        bg.norm_mode = "both"
    with torch.no_grad():
        z = model.encode(bg)
        _, gl = ops.decoder_bce_graphs(z, None, bg, graph_loss=True)
    got = model.score_graphs(ds, fused=True)
    a, b = got.loss.cpu().numpy().astype(np.float64), gl.cpu().numpy().astype(np.float64)
    err = np.nanmax(np.abs(a - b) / np.maximum(1.0, np.abs(b)))
    print(f"loss vs decoder_bce_graphs, norm={norm}: {err:.3e}")
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.isnan(a[[5, 50]]).all()
    assert err < TOL


# ------------------------------------------------------------------ 5. independence, bit for bit
def same(a, b):
    return all(torch.equal(x, y) or (x.is_floating_point() and torch.equal(torch.nan_to_num(x, nan=-7.0), torch.nan_to_num(y, nan=-7.0)))
               for x, y in zip(a, b))


def rows_of(scores, idx):
    return type(scores)(*(t[idx] for t in scores))


@pytest.mark.parametrize("storage,norm", [("uint8", "none"), ("float32", "both")])
def test_a_graphs_scores_depend_on_that_graph_alone(storage, norm, dev):
    from gae_dgl_amd import _lib, workloads
    gp, src, dst, X = workloads.zinc_like(2000, seed=7)
    if storage == "float32":
        X = np.random.default_rng(4).standard_normal(X.shape).astype(np.float32)
    ds = make_ds(gp, dst, src, X, dev, storage)
    model = random_model([32, 16], norm, dev, seed=1)
    emb = model.embed_graphs(ds, fused=True)
    before = _lib.CALLS["gae_score_graphs"]
    full = model.score_graphs(ds, fused=True)
    assert _lib.CALLS["gae_score_graphs"] == before + 1
    assert torch.equal(emb, model.embed_graphs(ds, fused=True))                          # K19 is not disturbed
    assert int((full.n_pos > 0).sum()) == 2000 and bool(torch.isfinite(full.loss).all())
    assert same(full, model.score_graphs(ds, fused=True))                                # a second run
    assert _lib.CALLS["gae_score_graphs"] == before + 2
    rng = np.random.default_rng(5)
    perm = rng.permutation(2000)
    on = lambda ids: torch.from_numpy(np.asarray(ids)).to(dev)                           # noqa: E731
    assert same(model.score_graphs(ds.subset(perm), fused=True), rows_of(full, on(perm)))
    part = perm[:777]                                                                    # another grouping
    assert same(model.score_graphs(ds.subset(part), fused=True), rows_of(full, on(part)))
    for g in (0, 1, 17, 640, 1999):                                                      # each graph alone
        assert same(model.score_graphs(ds.subset([g]), fused=True), rows_of(full, on([g])))
    rep = np.array([5, 5, 7, 5, 1999, 0, 5, 7, 7, 1999] * 13)                            # repeats inside one call
    assert same(model.score_graphs(ds.subset(rep), fused=True), rows_of(full, on(rep)))


# ------------------------------------------------------------------ 6. the routes
def test_auto_scores_large_graphs_one_by_one(dev):
    from gae_dgl_amd import _lib, metrics, ops
    from gae_dgl_amd._lib import GaeHipError
    rng = np.random.default_rng(21)
    sizes = rng.integers(6, 39, 500)
    big = [3, 250, 499]
    sizes[big] = 70
    gp, rows, cols = R.molecule_set(rng, sizes)
    X = (rng.random((int(gp[-1]), 39)) < 0.15).astype(np.float32)
    ds = make_ds(gp, rows, cols, X, dev)
    model = random_model([32, 16], "none", dev, seed=3)
    before = _lib.CALLS["gae_score_graphs"]
    out = model.score_graphs(ds, fused="auto")
    assert _lib.CALLS["gae_score_graphs"] == before + 1 and ops.score_graphs.last_request["n_out"] == 497
    small = np.setdiff1d(np.arange(500), big)
    assert same(rows_of(out, torch.from_numpy(small).to(dev)), model.score_graphs(ds.subset(small), fused=True))
    bg = ds.batch(big)                                               # the large ones, as the route batches them
    with torch.no_grad():
        z = model.encode(bg)
    indptr, indices = bg.csr()
    for k, g in enumerate(big):
        r0, r1 = 70 * k, 70 * (k + 1)
        e0, e1 = int(indptr[r0]), int(indptr[r1])
        ref = metrics.graph_scores_dense(z[r0:r1], (indptr[r0:r1 + 1].long() - e0, indices[e0:e1].long() - r0), True)
        for f in out._fields:
            v = float(getattr(out, f)[g])
            want = float(torch.tensor(ref[f], dtype=getattr(out, f).dtype))
            assert v == want or (np.isnan(v) and np.isnan(want)), (g, f, v, want)
        assert ref["n_pos"] > 0 and 0.0 <= ref["auc"] <= 1.0
    with pytest.raises(GaeHipError, match="70"):
        model.score_graphs(ds, fused=True)


def test_a_wide_model_takes_the_chunked_route(dev):
    from gae_dgl_amd import _lib, ops
    from gae_dgl_amd._lib import GaeHipError
    gp, rows, cols, X, _, _ = R.band_fixture()
    indptr, indices = R.csr_rows(int(gp[-1]), rows, cols)
    ds = make_ds(gp, rows, cols, X, dev, "float32")
    model = random_model([128, 16], "none", dev, seed=4)
    Ws, bs = params_of(model)
    _, logits = R.set_scores(gp, indptr, indices, X, Ws, bs, "none")
    bands, delta, open_pairs, pairs = R.band_totals(gp, indptr, indices, logits)
    print(f"wide model: {open_pairs} of {pairs} pairs open")
    before = _lib.CALLS["gae_score_graphs"]
    got = model.score_graphs(ds, fused="auto", batch_size=128)
    assert _lib.CALLS["gae_score_graphs"] == before + 3                       # 300 graphs in chunks of 128, no layers
    assert ops.score_graphs.last_request["widths"] == [] and ops.score_graphs.last_request["f_in"] == 16
    check_band(got, bands, f"39 -> 128 -> 16 chunked, delta={delta:.3e}")
    with pytest.raises(GaeHipError, match="128"):
        model.score_graphs(ds, fused=True)


def test_vgae_scores_mu(dev):
    from gae_dgl_amd import ops
    from gae_dgl_amd.vgae import VGAE
    rng = np.random.default_rng(9)
    gp, rows, cols = R.molecule_set(rng, rng.integers(4, 39, 120))
    X = (rng.random((int(gp[-1]), 39)) < 0.15).astype(np.float32)
    ds = make_ds(gp, rows, cols, X, dev)
    torch.manual_seed(0)
    model = VGAE(39, [32, 16]).to(dev)
    bg = ds.batch(np.arange(120))
    h = bg.ndata['h']
    got = model.score_graphs(bg)
    assert bg.ndata['h'] is h
    with torch.no_grad():
        mu, _ = model.encode(bg)
    bg.ndata['h'] = h
    indptr, indices = bg.csr()
    ref = ops.score_graphs(bg.graph_ptr(), indptr, indices, mu.contiguous())
    assert same(got, ref) and int((got.n_pos > 0).sum()) == 120


def test_parameters_grads_and_ndata_are_untouched(dev):
    from gae_dgl_amd import workloads
    gp, src, dst, X = workloads.zinc_like(600, seed=3)
    ds = make_ds(gp, dst, src, X, dev)
    model = random_model([32, 16], "none", dev, seed=6)
    params = list(model.parameters())
    params[1].requires_grad_(False)
    for p in params:
        p.grad = torch.randn_like(p)
    snap = [(p.detach().clone(), p.grad.clone(), p.requires_grad, p.grad.data_ptr()) for p in params]
    ids = np.arange(100, 400)
    bg = ds.batch(ids)
    h = bg.ndata['h']
    h0 = h.clone()
    keys = set(bg.ndata)
    from_set = model.score_graphs(ds.subset(ids), fused=True)
    for fused in (True, "auto", False):
        out = model.score_graphs(bg, fused=fused)
        assert not out.loss.requires_grad and out.loss.shape == (300,)
        assert bg.ndata['h'] is h and torch.equal(h, h0) and set(bg.ndata) == keys
        if fused is False:
            assert torch.equal(out.n_pos, from_set.n_pos) and float((out.auc - from_set.auc).abs().max()) < 0.02
        else:
            assert same(out, from_set)               # fp32 rows of a batch hold the same 0 / 1 values: the same bits
    model.score_graphs(ds, fused=False, batch_size=256)
    for p, (v, g, rg, gptr) in zip(params, snap):
        assert torch.equal(p.detach(), v) and torch.equal(p.grad, g) and p.requires_grad == rg and p.grad.data_ptr() == gptr


# ------------------------------------------------------------------ 7. the scripts
def test_train_inductive_prints_and_records_validation_metrics(tmp_path, capsys, dev):
    import gae_dgl_amd as G
    from gae_dgl_amd import metrics, train_inductive as TI
    from gae_dgl_amd.dataset import DeviceGraphDataset
    TI.main(["--hidden_dims", "32", "16", "--synthetic", "3000", "-b", "128", "-e", "2", "--seed", "0", "--no_plot",
             "-s", str(tmp_path), "--val_metrics"])
    text = capsys.readouterr().out
    lines = [l for l in text.splitlines() if l.startswith("Epoch:")]
    assert len(lines) == 2 and all("| Val AUC: " in l and "| Val AP: " in l and "| Val loss (no dropout): " in l for l in lines)
    vm = TI.main.val_metrics
    assert set(vm) == {"auc", "ap", "loss"} and all(len(v) == 2 for v in vm.values())
    assert 0.5 < vm["auc"][-1] <= 1.0 and 0.0 < vm["ap"][-1] <= 1.0 and np.isfinite(vm["loss"][-1])
    assert f"Val AUC: {vm['auc'][-1]:.4f}" in lines[-1]
    # a fresh model from the checkpoint, the same split
    model = G.GAE(39, [32, 16])
    model.load_state_dict(torch.load(os.path.join(str(tmp_path), "ep01.pkl"), map_location="cpu"))
    model = model.to(dev)
    ds = DeviceGraphDataset.synthetic_zinc(3000, seed=0, device=dev)
    np.random.seed(0)
    order = np.random.permutation(3000)
    fresh = metrics.graph_score_summary(model.score_graphs(ds.subset(ds.ids[order[:300]])))
    assert fresh["auc"] == vm["auc"][-1] and fresh["ap"] == vm["ap"][-1] and fresh["loss"] == vm["loss"][-1]
    # without the flag nothing changes
    TI.main(["--hidden_dims", "32", "16", "--synthetic", "600", "-b", "128", "-e", "1", "--seed", "0", "--no_plot",
             "-s", str(tmp_path)])
    assert TI.main.val_metrics is None and "Val AUC" not in capsys.readouterr().out


def test_embed_script_writes_the_score_table(tmp_path, dev):
    import gae_dgl_amd as G
    from gae_dgl_amd import embed as E, train_inductive as TI
    from gae_dgl_amd.dataset import DeviceGraphDataset
    TI.main(["--hidden_dims", "32", "16", "--synthetic", "600", "-b", "128", "-e", "1", "--seed", "0", "--no_plot",
             "-s", str(tmp_path)])
    ckpt = os.path.join(str(tmp_path), "ep00.pkl")
    feats, table = os.path.join(str(tmp_path), "f.npy"), os.path.join(str(tmp_path), "s.npy")
    base = ["--checkpoint", ckpt, "--hidden_dims", "32", "16", "--synthetic", "600", "--seed", "0"]
    E.main(base + ["--out", feats, "--scores", table])
    plain = os.path.join(str(tmp_path), "g.npy")
    E.main(base + ["--out", plain])
    assert np.array_equal(np.load(feats), np.load(plain))                     # the feature output is unchanged
    t = np.load(table)
    assert t.shape == (600, 5) and t.dtype == np.float64
    model = G.GAE(39, [32, 16])
    model.load_state_dict(torch.load(ckpt, map_location="cpu"))
    sc = model.to(dev).score_graphs(DeviceGraphDataset.synthetic_zinc(600, seed=0, device=dev))
    want = torch.stack([sc.loss.double(), sc.auc, sc.ap, sc.n_pos.double(), sc.n_neg.double()], 1).cpu().numpy()
    assert np.array_equal(t, want, equal_nan=True) and np.isfinite(t[:, 1]).all()
