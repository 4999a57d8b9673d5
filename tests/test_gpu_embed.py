"""GAE.embed_graphs / ops.embed_graphs (K19, gae_embed_graphs): the molecule feature [mean | sum | max] of a whole
resident set from one fused launch -- against the reference's own vectors, against the fp64 oracle (oracle.gae_encode
followed by oracle.segment_readout) at the project's tolerance, bit for bit across subsets / positions / repeats / runs,
against the chunked batch -> encode -> readout route, and through the command line."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def O():
    from oracle import gae_oracle
    return gae_oracle


def rel_err(a, b):
    """tests/test_gpu_parity.py::rel_err: max abs difference over max(1, max |reference|)"""
    a = torch.as_tensor(a).detach().double().cpu(); b = torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    if b.numel() == 0:
        return 0.0
    return float((a - b).abs().max() / b.abs().max().clamp(min=1.0))


def oracle_features(gp, src, dst, X, model, norm):
    """fp64: oracle.gae_encode on the whole block-diagonal set, then oracle.segment_readout"""
    n = int(gp[-1])
    ip, ix = O().csr_from_coo(src, dst, n)
    Ws = [l.apply_mod.linear.weight.detach().double().cpu() for l in model.layers]
    bs = [l.apply_mod.linear.bias.detach().double().cpu() for l in model.layers]
    nv = O().norm_from_in_degrees(O().in_degrees(dst, n)) if norm == "both" else None
    Z = O().gae_encode(ip, ix, torch.as_tensor(np.asarray(X)).double(), Ws, bs, nv)
    return O().segment_readout(Z.numpy(), gp)


def make_model(hidden, norm, dev, seed=0, f_in=39):
    import gae_dgl_amd as G
    torch.manual_seed(seed)
    model = G.GAE(f_in, hidden, norm=None if norm == "none" else norm)
    with torch.no_grad():
        for l in model.layers:                       # biases large enough to matter
            l.apply_mod.linear.bias.uniform_(-0.5, 0.5)
    return model.to(dev)


def random_set(rng, sizes, binary=True, directed=False, hub=None):
    """a molecule-like set with the given node counts: a random tree per graph plus a few extra bonds, both directions
    (``directed``: random directed edges with duplicates and self loops instead); ``hub`` = (graph, node, entries):
    that many extra in-edges of one node from random nodes of its graph (duplicates)"""
    sizes = np.asarray(sizes, dtype=np.int64)
    gp = np.zeros(len(sizes) + 1, np.int64); np.cumsum(sizes, out=gp[1:])
    src, dst = [], []
    for g, n in enumerate(sizes):
        n = int(n)
        if n < 2 and not directed:
            continue
        if n == 0:
            continue
        if directed:
            e = int(rng.integers(0, 3 * n + 1))
            s = rng.integers(0, n, e); d = rng.integers(0, n, e)
            if e > 4:
                s[:2] = s[2:4]; d[:2] = d[2:4]       # duplicate edges
                s[4] = d[4]                           # a self loop
        else:
            child = np.arange(1, n); parent = child - np.minimum(rng.integers(1, 4, n - 1), child)
            extra = int(rng.integers(0, 4))
            a = np.concatenate([child, rng.integers(0, n, extra)]); b = np.concatenate([parent, rng.integers(0, n, extra)])
            keep = a != b
            a, b = a[keep], b[keep]
            s = np.stack([a, b], 1).reshape(-1); d = np.stack([b, a], 1).reshape(-1)
        src.append(s + gp[g]); dst.append(d + gp[g])
    if hub is not None:
        g, node, entries = hub
        src.append(gp[g] + rng.integers(0, sizes[g], entries)); dst.append(np.full(entries, gp[g] + node))
    src = np.concatenate(src).astype(np.int64) if src else np.zeros(0, np.int64)
    dst = np.concatenate(dst).astype(np.int64) if dst else np.zeros(0, np.int64)
    N = int(gp[-1])
    if binary:
        X = (rng.random((N, 39)) < 0.15).astype(np.float32)
    else:
        X = rng.standard_normal((N, 39)).astype(np.float32)
    return gp, src, dst, X


def make_ds(arrays, dev, storage):
    from gae_dgl_amd.dataset import DeviceGraphDataset
    gp, src, dst, X = arrays
    ds = DeviceGraphDataset(gp, src, dst, X, device=dev, feat_storage=storage)
    if storage == "float32":
        assert ds.feat.dtype == torch.float32 and ds.feat.stride(0) > ds.feat.shape[1]
        ds.feat._base[:, ds.feat.shape[1]:] = float("nan")      # the pad column is never read as data
    else:
        assert ds.feat.dtype == torch.uint8 and ds.feat.stride(0) == 48
    return ds


@pytest.fixture(scope="module")
def zinc2000():
    from gae_dgl_amd import workloads
    return workloads.zinc_like(2000, seed=7)


# ------------------------------------------------------------------ 1. pinned to the reference
def test_golden_molecules_match_the_reference_embedding(dev):
    """the eight golden molecules as a resident dataset, the model of the reference's state dict: the fused launch ==
    segment_readout of the reference's own Z"""
    import gae_dgl_amd as G
    from gae_dgl_amd.dataset import DeviceGraphDataset
    parts = load_golden("mol8_parts"); whole = load_golden("mol8")
    ng = int(parts["n_graphs"])
    sizes = [int(parts[f"g{i}/n"]) for i in range(ng)]
    gp = np.zeros(ng + 1, np.int64); np.cumsum(sizes, out=gp[1:])
    src = np.concatenate([parts[f"g{i}/src"] + gp[i] for i in range(ng)])
    dst = np.concatenate([parts[f"g{i}/dst"] + gp[i] for i in range(ng)])
    X = np.concatenate([parts[f"g{i}/X"] for i in range(ng)])
    assert np.array_equal(X, whole["X"]) and int(gp[-1]) == int(whole["n"])
    ds = DeviceGraphDataset(gp, src, dst, X, device=dev)
    model = G.GAE(X.shape[1], [int(h) for h in whole["hidden"]])
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in whole.items() if k.startswith("sd/")})
    model = model.to(dev)
    out = model.embed_graphs(ds, fused=True)
    ref = O().segment_readout(whole["Z"], gp)
    err = rel_err(out, ref)
    print(f"mol8: fused embedding vs the reference's Z: {err:.3e}")
    assert out.shape == (ng, 3 * whole["Z"].shape[1]) and out.dtype == torch.float32
    assert err < TOL


# ------------------------------------------------------------------ 2. against the fp64 oracle, fused=True throughout
@pytest.mark.parametrize("storage", ["uint8", "float32"])
@pytest.mark.parametrize("norm", ["none", "both"])
@pytest.mark.parametrize("hidden", [[32, 16], [16], [64, 32, 16], [32, 32, 32, 8]], ids=lambda h: "x".join(map(str, h)))
def test_zinc_like_molecules_match_the_oracle(hidden, norm, storage, zinc2000, dev):
    gp, src, dst, X = zinc2000
    if storage == "float32":                         # non-binary values
        X = np.random.default_rng(3).standard_normal(X.shape).astype(np.float32)
    ds = make_ds((gp, src, dst, X), dev, storage)
    model = make_model(hidden, norm, dev, seed=len(hidden))
    out = model.embed_graphs(ds, fused=True)
    ref = oracle_features(gp, src, dst, X, model, norm)
    err = rel_err(out, ref)
    print(f"zinc_like 2000 x {hidden} norm={norm} {storage}: {err:.3e}")
    assert out.shape == (2000, 3 * hidden[-1])
    assert err < TOL


@pytest.mark.parametrize("storage", ["uint8", "float32"])
@pytest.mark.parametrize("norm", ["none", "both"])
def test_directed_duplicates_and_self_loops_match_the_oracle(norm, storage, dev):
    rng = np.random.default_rng(11)
    arrays = random_set(rng, rng.integers(1, 40, 300), binary=storage == "uint8", directed=True)
    ds = make_ds(arrays, dev, storage)
    assert not ds.symmetric
    model = make_model([32, 16], norm, dev, seed=5)
    err = rel_err(model.embed_graphs(ds, fused=True), oracle_features(*arrays, model, norm))
    print(f"directed, duplicates, self loops norm={norm} {storage}: {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("storage", ["uint8", "float32"])
@pytest.mark.parametrize("norm", ["none", "both"])
def test_edge_shapes_match_the_oracle(norm, storage, dev):
    """empty graphs, one-atom graphs without edges, graphs of exactly 64 nodes, a hub row longer than 64 entries through
    duplicates -- first, last and in the middle of the set"""
    rng = np.random.default_rng(13)
    sizes = [0, 1, 64, 5, 0, 0, 1, 64, 64, 12, 30, 1, 63, 2, 64, 0]
    arrays = random_set(rng, sizes, binary=storage == "uint8", hub=(9, 3, 80))
    gp, src, dst, X = arrays
    ds = make_ds(arrays, dev, storage)
    assert int((ds.indptr[1:] - ds.indptr[:-1]).max()) > 64              # the hub row
    model = make_model([32, 16], norm, dev, seed=9)
    out = model.embed_graphs(ds, fused=True)
    ref = oracle_features(gp, src, dst, X, model, norm)
    err = rel_err(out, ref)
    print(f"edge shapes norm={norm} {storage}: {err:.3e}")
    assert err < TOL
    for g, n in enumerate(sizes):
        if n == 0:
            assert float(out[g].abs().max()) == 0.0                       # zeros in all three blocks
        if n == 1:
            d = 16
            assert torch.equal(out[g, :d], out[g, d:2 * d]) and torch.equal(out[g, :d], out[g, 2 * d:])


def test_every_graph_empty_and_an_empty_selection(dev):
    rng = np.random.default_rng(2)
    arrays = random_set(rng, [3, 0, 0, 4])
    ds = make_ds(arrays, dev, "uint8")
    model = make_model([32, 16], "none", dev)
    out = model.embed_graphs(ds.subset([1, 2, 1]), fused=True)
    assert out.shape == (3, 48) and float(out.abs().max()) == 0.0
    assert model.embed_graphs(ds.subset([]), fused=True).shape == (0, 48)


# ------------------------------------------------------------------ 3. independence, bit for bit
@pytest.mark.parametrize("storage,norm", [("uint8", "none"), ("float32", "both")])
def test_a_graphs_row_depends_on_that_graph_alone(storage, norm, zinc2000, dev):
    gp, src, dst, X = zinc2000
    if storage == "float32":
        X = np.random.default_rng(4).standard_normal(X.shape).astype(np.float32)
    ds = make_ds((gp, src, dst, X), dev, storage)
    model = make_model([32, 16], norm, dev, seed=1)
    full = model.embed_graphs(ds, fused=True)
    assert torch.equal(full, model.embed_graphs(ds, fused=True))                       # a second run
    rng = np.random.default_rng(5)
    perm = rng.permutation(2000)
    assert torch.equal(model.embed_graphs(ds.subset(perm), fused=True), full[torch.from_numpy(perm).to(dev)])
    part = perm[:777]                                                                   # another grouping
    assert torch.equal(model.embed_graphs(ds.subset(part), fused=True), full[torch.from_numpy(part).to(dev)])
    for g in (0, 1, 17, 640, 1999):                                                     # each graph alone
        assert torch.equal(model.embed_graphs(ds.subset([g]), fused=True)[0], full[g])
    rep = np.array([5, 5, 7, 5, 1999, 0, 5, 7, 7, 1999] * 13)                           # repeats inside one call
    assert torch.equal(model.embed_graphs(ds.subset(rep), fused=True), full[torch.from_numpy(rep).to(dev)])


# ------------------------------------------------------------------ 4. the routes agree
@pytest.mark.parametrize("norm", ["none", "both"])
def test_fused_and_chunked_routes_agree(norm, zinc2000, dev):
    gp, src, dst, X = zinc2000
    ds = make_ds((gp, src, dst, X), dev, "uint8")
    model = make_model([32, 16], norm, dev, seed=2)
    a = model.embed_graphs(ds, fused=True)
    for bs in (4096, 128, 777):
        b = model.embed_graphs(ds, fused=False, batch_size=bs)
        err = max(rel_err(a, b), rel_err(b, a))
        print(f"fused vs chunked (batch {bs}) norm={norm}: {err:.3e}")
        assert err < TOL
    perm = np.random.default_rng(1).permutation(2000)[:300]
    assert rel_err(model.embed_graphs(ds.subset(perm), fused=False, batch_size=64), a[torch.from_numpy(perm).to(dev)]) < TOL


def _set_with_three_large_graphs(dev):
    rng = np.random.default_rng(21)
    sizes = rng.integers(6, 39, 500)
    big = [3, 250, 499]
    sizes[big] = 70
    arrays = random_set(rng, sizes)
    return arrays, make_ds(arrays, dev, "uint8"), big


def test_auto_takes_the_kernel_for_every_graph_it_can(dev):
    from gae_dgl_amd import _lib, ops
    from gae_dgl_amd._lib import GaeHipError
    arrays, ds, big = _set_with_three_large_graphs(dev)
    model = make_model([32, 16], "none", dev, seed=3)
    before = _lib.CALLS["gae_embed_graphs"]
    out = model.embed_graphs(ds, fused="auto")
    assert _lib.CALLS["gae_embed_graphs"] == before + 1
    assert ops.embed_graphs.last_request["n_out"] == 497            # the graph_ids the wrapper passed
    ref = oracle_features(*arrays, model, "none")
    err = rel_err(out, ref)
    print(f"auto, 497 + 3 graphs: {err:.3e}")
    assert out.shape == (500, 48) and err < TOL
    small = np.setdiff1d(np.arange(500), big)
    assert torch.equal(out[torch.from_numpy(small).to(dev)], model.embed_graphs(ds.subset(small), fused=True))
    with pytest.raises(GaeHipError, match="70"):
        model.embed_graphs(ds, fused=True)
    assert _lib.CALLS["gae_embed_graphs"] == before + 2             # (the subset call above; the refusal launched nothing)


def test_auto_with_a_wide_model_takes_the_chunked_route(zinc2000, dev):
    from gae_dgl_amd import _lib
    from gae_dgl_amd._lib import GaeHipError
    gp, src, dst, X = zinc2000
    ds = make_ds((gp, src, dst, X), dev, "uint8")
    model = make_model([128, 64], "none", dev, seed=4)
    before = _lib.CALLS["gae_embed_graphs"]
    out = model.embed_graphs(ds, fused="auto", batch_size=512)
    assert _lib.CALLS["gae_embed_graphs"] == before
    err = rel_err(out, oracle_features(gp, src, dst, X, model, "none"))
    print(f"auto, 39 -> 128 -> 64: {err:.3e}")
    assert out.shape == (2000, 192) and err < TOL
    with pytest.raises(GaeHipError, match="128"):
        model.embed_graphs(ds, fused=True)


# ------------------------------------------------------------------ 5. nothing else changes
def test_parameters_and_ndata_are_untouched(zinc2000, dev):
    gp, src, dst, X = zinc2000
    ds = make_ds((gp, src, dst, X), dev, "uint8")
    model = make_model([32, 16], "none", dev, seed=6)
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
    from_set = model.embed_graphs(ds.subset(ids), fused=True)
    for fused in (True, "auto", False):
        out = model.embed_graphs(bg, fused=fused)
        assert not out.requires_grad and out.shape == (300, 48)
        assert bg.ndata['h'] is h and torch.equal(h, h0) and set(bg.ndata) == keys
        if fused is False:
            assert rel_err(out, from_set) < TOL
        else:
            assert torch.equal(out, from_set)        # fp32 rows of a batch hold the same 0 / 1 values: the same bits
    model.embed_graphs(ds, fused=False, batch_size=512)
    for p, (v, g, rg, gptr) in zip(params, snap):
        assert torch.equal(p.detach(), v) and torch.equal(p.grad, g) and p.requires_grad == rg and p.grad.data_ptr() == gptr
    assert not from_set.requires_grad


# ------------------------------------------------------------------ 6. the script, end to end
def test_script_embeds_a_checkpoint_of_train_inductive(tmp_path, dev):
    import gae_dgl_amd as G
    from gae_dgl_amd import embed as E, train_inductive as TI
    from gae_dgl_amd.dataset import DeviceGraphDataset
    TI.main(["--hidden_dims", "32", "16", "--synthetic", "600", "-b", "128", "-e", "1", "--seed", "0", "--no_plot",
             "-s", str(tmp_path)])
    ckpt = os.path.join(str(tmp_path), "ep00.pkl")
    assert os.path.exists(ckpt)
    path = os.path.join(str(tmp_path), "features.npy")
    E.main(["--checkpoint", ckpt, "--hidden_dims", "32", "16", "--synthetic", "600", "--seed", "0", "--out", path])
    feats = np.load(path)
    assert feats.shape == (600, 48) and feats.dtype == np.float32
    model = G.GAE(39, [32, 16])
    model.load_state_dict(torch.load(ckpt, map_location="cpu"))
    model = model.to(dev)
    ds = DeviceGraphDataset.synthetic_zinc(600, seed=0, device=dev)
    assert np.array_equal(feats, model.embed_graphs(ds).cpu().numpy())
    assert np.isfinite(feats).all() and float(np.abs(feats).max()) > 0
    off = os.path.join(str(tmp_path), "features_off.npy")
    E.main(["--checkpoint", ckpt, "--hidden_dims", "32", "16", "--synthetic", "600", "--seed", "0", "--out", off,
            "--fused", "off", "--batch_size", "128"])
    assert rel_err(np.load(off), feats) < TOL
