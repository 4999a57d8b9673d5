"""The differentiable molecule feature: gae_embed_graphs_bwd (K21) behind ops.embed_graphs / GAE.embed_graphs(grad=True),
gae_segment_readout_bwd behind ops.segment_readout, and python -m gae_dgl_amd.finetune -- weight gradients against the
fp64 reference of tests/embed_grad_ref.py at the project's fp32-gradient tolerance (rel_err <= 1e-5; the reference
asserts on every input that its tie rule does not show in them), the tie rule itself on dZ, bit-for-bit repeats, frozen
parameters, the three routes of grad=True, one training step end to end and the script."""
import os

import numpy as np
import pytest
import torch

import embed_grad_ref as R
from embed_grad_ref import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-5
ENCODERS = [[32, 16], [16], [64, 32, 16], [32, 32, 32, 8]]
ENC_IDS = lambda h: "x".join(map(str, h))      # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def zinc2000():
    from gae_dgl_amd import workloads
    return workloads.zinc_like(2000, seed=7)


def make_model(hidden, norm, dev, seed=0, f_in=39, dead=False):
    import gae_dgl_amd as G
    torch.manual_seed(seed)
    model = G.GAE(f_in, hidden, norm=None if norm == "none" else norm)
    with torch.no_grad():
        for k, l in enumerate(model.layers):
            if dead and k < len(model.layers) - 1:
                l.apply_mod.linear.bias.uniform_(-1.5, 0.0)      # a good share of the ReLU units is dead
            else:
                l.apply_mod.linear.bias.uniform_(-0.5, 0.5)
    return model.to(dev)


def random_set(rng, sizes, binary=True, directed=False, hub=None):
    """tests/test_gpu_embed.py::random_set: a molecule-like set with the given node counts -- a random tree per graph
    plus a few extra bonds, both directions (``directed``: random directed edges with duplicates and self loops);
    ``hub`` = (graph, node, entries): that many extra in-edges of one node from random nodes of its graph"""
    sizes = np.asarray(sizes, dtype=np.int64)
    gp = np.zeros(len(sizes) + 1, np.int64); np.cumsum(sizes, out=gp[1:])
    src, dst = [], []
    for g, n in enumerate(sizes):
        n = int(n)
        if n == 0 or (n < 2 and not directed):
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
    X = (rng.random((N, 39)) < 0.15).astype(np.float32) if binary else rng.standard_normal((N, 39)).astype(np.float32)
    return gp, src, dst, X


def make_ds(arrays, dev, storage):
    from gae_dgl_amd.dataset import DeviceGraphDataset
    gp, src, dst, X = arrays
    ds = DeviceGraphDataset(gp, src, dst, X, device=dev, feat_storage=storage)
    assert ds.feat.dtype == (torch.float32 if storage == "float32" else torch.uint8)
    return ds


def params_of(model):
    return [l.apply_mod.linear.weight for l in model.layers] + [l.apply_mod.linear.bias for l in model.layers]


def fused_grads(model, data, d_out, **kw):
    """(features, grads of weights then biases) of sum(features * d_out) through GAE.embed_graphs(grad=True)"""
    for p in model.parameters():
        p.grad = None
    out = model.embed_graphs(data, grad=True, **kw)
    (out * d_out).sum().backward()
    grads = [None if p.grad is None else p.grad.clone() for p in params_of(model)]
    return out.detach(), grads


def check_against_reference(tag, arrays, model, norm, ds, dev, graph_ids=None, seed=0, **kw):
    B = len(arrays[0]) - 1 if graph_ids is None else len(graph_ids)
    d = model.layers[-1].apply_mod.linear.out_features
    d_out = torch.randn(B, 3 * d, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
    F, dWs, dbs = R.encoder_grads(*arrays, model, norm, d_out, graph_ids)
    data = ds if graph_ids is None else ds.subset(graph_ids)
    out, grads = fused_grads(model, data, d_out.to(dev), fused=True, **kw)
    errs = [rel_err(g, r) for g, r in zip(grads, dWs + dbs)]
    print(f"{tag}: features {rel_err(out, F):.3e} | dW {['%.2e' % e for e in errs[:len(dWs)]]} | "
          f"db {['%.2e' % e for e in errs[len(dWs):]]} | max |g| {max(float(r.abs().max()) for r in dWs + dbs):.3g}")
    assert rel_err(out, F) <= TOL
    assert max(errs) <= TOL, errs
    return grads


# ------------------------------------------------------------------ 1. the readout's own backward, the tie rule
@pytest.mark.parametrize("d", [1, 16, 48, 100])
def test_segment_readout_bwd_matches_the_reference_and_its_tie_rule(d, dev):
    from gae_dgl_amd import ops
    rng = np.random.default_rng(d)
    sizes = [0, 1, 2, 63, 64, 65, 300, 0, 5]
    gp = np.zeros(len(sizes) + 1, np.int64); np.cumsum(sizes, out=gp[1:])
    Z = rng.standard_normal((int(gp[-1]), d)).astype(np.float32)
    # rows duplicated on purpose: the maximum of a column is attained twice (graph of 63) and three times (graph of 300)
    g63, g300 = int(gp[3]), int(gp[6])
    top = Z[g63:g63 + 63].argmax(0)
    Z[g63 + 40] = Z[g63 + top, np.arange(d)]          # row 40 ties the maximum of every column
    Z[g63 + 7] = Z[g63 + 40]                          # and so does row 7
    Z[g300 + 250] = Z[g300:g300 + 300].max(0); Z[g300 + 100] = Z[g300 + 250]; Z[g300 + 299] = Z[g300 + 250]
    Z[int(gp[2])] = Z[int(gp[2]) + 1]                 # the graph of two rows: both equal
    d_out = rng.standard_normal((len(sizes), 3 * d)).astype(np.float32)
    ref = R.readout_dz(Z, gp, d_out, "first")
    assert float((ref - R.readout_dz(Z, gp, d_out, "last")).abs().max()) > 0.1      # the rule is visible here
    Zd = torch.from_numpy(Z).to(dev).requires_grad_(True)
    out = ops.segment_readout(Zd, torch.from_numpy(gp).to(dev))
    assert out.requires_grad
    out.backward(torch.from_numpy(d_out).to(dev))
    err = float((Zd.grad.double().cpu() - ref).abs().max())
    print(f"segment_readout_bwd d={d}: max abs error {err:.3e}")
    assert Zd.grad.shape == Z.shape and err <= 1e-6
    # the whole d_max on the lowest row attaining the maximum: d_mean = d_sum = 0 leaves exactly one entry per column
    only_max = d_out.copy(); only_max[:, :2 * d] = 0.0
    dz = ops.segment_readout_bwd(Zd.detach(), torch.from_numpy(gp).to(dev), torch.from_numpy(only_max).to(dev)).cpu().numpy()
    for g, lo in ((3, g63), (6, g300)):
        block = dz[lo:lo + sizes[g]]
        first = (Z[lo:lo + sizes[g]] == Z[lo:lo + sizes[g]].max(0)).argmax(0)
        assert (np.count_nonzero(block, axis=0) <= 1).all()
        assert np.array_equal(block[first, np.arange(d)], only_max[g, 2 * d:])
    assert np.array_equal(dz[int(gp[2])], only_max[2, 2 * d:]) and not dz[int(gp[2]) + 1].any()
    # forward values and the launch are what they were; no gradient without one asked for
    with torch.no_grad():
        assert torch.equal(ops.segment_readout(Zd, torch.from_numpy(gp).to(dev)), out.detach())
    assert not ops.segment_readout(Zd.detach(), torch.from_numpy(gp).to(dev)).requires_grad


# ------------------------------------------------------------------ 2. K21 against fp64
@pytest.mark.parametrize("storage", ["uint8", "float32"])
@pytest.mark.parametrize("norm", ["none", "both"])
@pytest.mark.parametrize("hidden", ENCODERS, ids=ENC_IDS)
def test_zinc_like_gradients_match_fp64(hidden, norm, storage, zinc2000, dev):
    gp, src, dst, X = zinc2000
    if storage == "float32":                         # (d) non-binary values
        X = np.random.default_rng(3).standard_normal(X.shape).astype(np.float32)
    ds = make_ds((gp, src, dst, X), dev, storage)
    model = make_model(hidden, norm, dev, seed=len(hidden))
    check_against_reference(f"zinc_like 2000 x {hidden} norm={norm} {storage}", (gp, src, dst, X), model, norm, ds, dev)


@pytest.mark.parametrize("norm", ["none", "both"])
@pytest.mark.parametrize("hidden", [[32, 16], [64, 32, 16]], ids=ENC_IDS)
def test_dead_relu_units(hidden, norm, zinc2000, dev):
    """(e) hidden biases in (-1.5, 0): most pre-activations are negative, the masks matter"""
    gp, src, dst, X = zinc2000
    ds = make_ds((gp, src, dst, X), dev, "uint8")
    model = make_model(hidden, norm, dev, seed=7, dead=True)
    check_against_reference(f"dead units {hidden} norm={norm}", (gp, src, dst, X), model, norm, ds, dev, seed=1)


@pytest.mark.parametrize("storage", ["uint8", "float32"])
@pytest.mark.parametrize("norm", ["none", "both"])
@pytest.mark.parametrize("hidden", ENCODERS, ids=ENC_IDS)
def test_directed_sets_with_duplicates_and_self_loops(hidden, norm, storage, dev):
    """(b) a symmetric set cannot see a missing transpose"""
    rng = np.random.default_rng(11)
    arrays = random_set(rng, rng.integers(1, 40, 300), binary=storage == "uint8", directed=True)
    ds = make_ds(arrays, dev, storage)
    assert not ds.symmetric
    model = make_model(hidden, norm, dev, seed=5, dead=len(hidden) == 2)
    check_against_reference(f"directed {hidden} norm={norm} {storage}", arrays, model, norm, ds, dev, seed=2)


@pytest.mark.parametrize("storage", ["uint8", "float32"])
@pytest.mark.parametrize("norm", ["none", "both"])
@pytest.mark.parametrize("hidden", ENCODERS, ids=ENC_IDS)
def test_edge_shapes(hidden, norm, storage, dev):
    """(c) groups that fill exactly 64 rows, a next graph that does not fit, a hub row of 40 entries (the CSR tail
    path, forward and transposed), graphs without edges, an empty graph; B = 11 is no multiple of the 4 slots of a wave
    and spans three blocks"""
    rng = np.random.default_rng(13)
    sizes = [0, 1, 2, 64, 63, 1, 64, 33, 31, 32, 32]
    arrays = random_set(rng, sizes, binary=storage == "uint8", hub=(7, 3, 40))
    ds = make_ds(arrays, dev, storage)
    assert int((ds.indptr[1:] - ds.indptr[:-1]).max()) >= 40
    model = make_model(hidden, norm, dev, seed=9)
    check_against_reference(f"edge shapes {hidden} norm={norm} {storage}", arrays, model, norm, ds, dev, seed=3)


def test_directed_hub_rows_take_the_tail_path_both_ways(dev):
    """a directed set in which one node lists 40 entries (with repeats) and another is listed by more than four rows:
    the aggregate's CSR tail and the transposed gather's mask path"""
    rng = np.random.default_rng(17)
    sizes = [20, 50, 7]
    gp, src, dst, X = random_set(rng, sizes, directed=True, hub=(1, 5, 40))
    fan = np.arange(10, 30)                                        # 20 rows of graph 1 list node 9; three of them twice
    src = np.concatenate([src, np.full(23, gp[1] + 9)]); dst = np.concatenate([dst, gp[1] + np.concatenate([fan, fan[:3]])])
    arrays = (gp, src, dst, X)
    ds = make_ds(arrays, dev, "uint8")
    for norm in ("none", "both"):
        model = make_model([32, 32, 16], norm, dev, seed=2)
        check_against_reference(f"hub rows norm={norm}", arrays, model, norm, ds, dev, seed=4)


# ------------------------------------------------------------------ 3. graph_ids
@pytest.mark.parametrize("norm", ["none", "both"])
def test_a_permuted_subset_with_a_repeat(norm, zinc2000, dev):
    gp, src, dst, X = zinc2000
    ds = make_ds((gp, src, dst, X), dev, "uint8")
    model = make_model([32, 16], norm, dev, seed=1)
    ids = np.random.default_rng(5).permutation(2000)[:301]
    ids[300] = ids[17]                                             # listed twice: contributes twice
    check_against_reference(f"graph_ids norm={norm}", (gp, src, dst, X), model, norm, ds, dev, graph_ids=ids, seed=6)


# ------------------------------------------------------------------ 4., 5. frozen parameters, reproducibility
def test_frozen_parameters_get_no_gradient_and_change_no_bits(zinc2000, dev):
    from gae_dgl_amd import _lib, ops
    gp, src, dst, X = zinc2000
    ds = make_ds((gp, src, dst, X), dev, "uint8")
    model = make_model([64, 32, 16], "both", dev, seed=3)
    d_out = torch.randn(2000, 48, generator=torch.Generator().manual_seed(8)).to(dev)
    _, full = fused_grads(model, ds, d_out, fused=True)
    before = _lib.CALLS["gae_embed_graphs_bwd"]
    _, again = fused_grads(model, ds, d_out, fused=True)
    assert _lib.CALLS["gae_embed_graphs_bwd"] == before + 1      # the backward is ONE call
    for a, b in zip(full, again):
        assert torch.equal(a, b)                                   # 5. same call, same bits
    ps = params_of(model)
    for p in ps:
        p.requires_grad_(False)
    ps[2].requires_grad_(True); ps[5].requires_grad_(True)         # the last layer alone
    _, last = fused_grads(model, ds, d_out, fused=True)
    assert ops.embed_graphs_bwd.last_request["want_weights"] == [False, False, True]
    for k, g in enumerate(last):
        if k in (2, 5):
            assert torch.equal(g, full[k])
        else:
            assert g is None
    ps[2].requires_grad_(False); ps[5].requires_grad_(False); ps[3].requires_grad_(True)       # one bias of layer 0
    _, one = fused_grads(model, ds, d_out, fused=True)
    assert [g is not None for g in one] == [False, False, False, True, False, False] and torch.equal(one[3], full[3])
    for p in ps:
        p.requires_grad_(False)
    out = model.embed_graphs(ds, fused=True, grad=True)
    assert not out.requires_grad                                   # nothing to train: today's single launch


def test_raw_wrapper_and_no_grad_behaviour(zinc2000, dev):
    from gae_dgl_amd import _lib, ops
    gp, src, dst, X = zinc2000
    ds = make_ds((gp, src, dst, X), dev, "float32")
    model = make_model([32, 16], "none", dev, seed=2)
    lins = [l.apply_mod.linear for l in model.layers]
    args = (ds.graph_ptr, ds.indptr, ds.indices, ds.feat, [l.weight for l in lins], [l.bias for l in lins], [1, 0])
    d_out = torch.randn(2000, 48, generator=torch.Generator().manual_seed(9)).to(dev)
    dWs, dbs = ops.embed_graphs_bwd(*args, d_out, max_graph_nodes=38)
    _, ref = fused_grads(model, ds, d_out, fused=True)
    for a, b in zip(dWs + dbs, ref):
        assert torch.equal(a, b)
    dWs, dbs = ops.embed_graphs_bwd(*args, d_out, want_weights=[False, True], want_biases=[True, False])
    assert dWs[0] is None and dbs[1] is None and torch.equal(dWs[1], ref[1]) and torch.equal(dbs[0], ref[2])
    # no graphs: zeros
    none = torch.zeros(0, dtype=torch.int64, device=dev)
    dWs, dbs = ops.embed_graphs_bwd(*args, d_out[:0], graph_ids=none, max_graph_nodes=0)
    assert all(float(g.abs().max()) == 0.0 for g in dWs + dbs)
    # a refused slot (graph id out of range) contributes nothing; the forward writes NaN for it
    ids = torch.tensor([3, 2000, 4], device=dev)
    a, _ = ops.embed_graphs_bwd(*args, d_out[:3].contiguous(), graph_ids=ids, max_graph_nodes=38)
    b, _ = ops.embed_graphs_bwd(*args, d_out[[0, 2]].contiguous(), graph_ids=ids[[0, 2]], max_graph_nodes=38)
    assert rel_err(a[0], b[0]) <= 1e-6 and rel_err(a[1], b[1]) <= 1e-6
    # under no_grad the call is today's single launch
    before = dict(_lib.CALLS)
    with torch.no_grad():
        out = ops.embed_graphs(*args)
    assert not out.requires_grad and _lib.CALLS["gae_embed_graphs"] == before.get("gae_embed_graphs", 0) + 1
    assert _lib.CALLS["gae_embed_graphs_bwd"] == before.get("gae_embed_graphs_bwd", 0)
    assert torch.equal(out, ops.embed_graphs(*args).detach())      # with a graph attached: the same bits


# ------------------------------------------------------------------ 6. forward values and the three routes
def _set_with_three_large_graphs(dev):
    rng = np.random.default_rng(21)
    sizes = rng.integers(6, 39, 500)
    big = [3, 250, 499]
    sizes[big] = 70
    arrays = random_set(rng, sizes)
    return arrays, make_ds(arrays, dev, "uint8"), big


def test_grad_true_forward_values_and_routes(dev):
    from gae_dgl_amd import _lib, ops
    from gae_dgl_amd._lib import GaeHipError
    arrays, ds, big = _set_with_three_large_graphs(dev)
    small = np.setdiff1d(np.arange(500), big)
    model = make_model([32, 16], "none", dev, seed=3)
    d_out = torch.randn(500, 48, generator=torch.Generator().manual_seed(10))
    F, dWs, dbs = R.encoder_grads(*arrays, model, "none", d_out)
    for fused in ("auto", False):
        plain = model.embed_graphs(ds, fused=fused, batch_size=128)
        before = (_lib.CALLS["gae_embed_graphs"], _lib.CALLS["gae_embed_graphs_bwd"])
        out, grads = fused_grads(model, ds, d_out.to(dev), fused=fused, batch_size=128)
        assert torch.equal(out, plain)                             # grad=True forward == grad=False, bit for bit
        assert rel_err(out, F) <= TOL
        errs = [rel_err(g, r) for g, r in zip(grads, dWs + dbs)]
        print(f"grad=True fused={fused}: {['%.2e' % e for e in errs]}")
        assert max(errs) <= TOL
        calls = (_lib.CALLS["gae_embed_graphs"] - before[0], _lib.CALLS["gae_embed_graphs_bwd"] - before[1])
        if fused == "auto":
            assert calls == (1, 1) and ops.embed_graphs.last_request["n_out"] == 497
            assert ops.embed_graphs_bwd.last_request["n_out"] == 497
        else:
            assert calls == (0, 0)
    sub = ds.subset(small)
    out, grads = fused_grads(model, sub, d_out[small].to(dev), fused=True)
    assert torch.equal(out, model.embed_graphs(sub, fused=True))
    Fs, dWs, dbs = R.encoder_grads(*arrays, model, "none", d_out[small], graph_ids=small)
    assert rel_err(out, Fs) <= TOL and max(rel_err(g, r) for g, r in zip(grads, dWs + dbs)) <= TOL
    with pytest.raises(GaeHipError, match="70"):
        model.embed_graphs(ds, fused=True, grad=True)


def test_a_wide_model_takes_the_chunked_route_under_auto(zinc2000, dev):
    from gae_dgl_amd import _lib
    from gae_dgl_amd._lib import GaeHipError
    gp, src, dst, X = zinc2000
    keep = 300
    arrays = (gp[:keep + 1], src[src < gp[keep]], dst[dst < gp[keep]], X[:gp[keep]])
    ds = make_ds(arrays, dev, "uint8")
    model = make_model([128, 64], "none", dev, seed=4)
    d_out = torch.randn(keep, 192, generator=torch.Generator().manual_seed(11))
    before = (_lib.CALLS["gae_embed_graphs"], _lib.CALLS["gae_embed_graphs_bwd"])
    out, grads = fused_grads(model, ds, d_out.to(dev), fused="auto", batch_size=128)
    assert (_lib.CALLS["gae_embed_graphs"], _lib.CALLS["gae_embed_graphs_bwd"]) == before
    F, dWs, dbs = R.encoder_grads(*arrays, model, "none", d_out)
    errs = [rel_err(g, r) for g, r in zip(grads, dWs + dbs)]
    print(f"auto, 39 -> 128 -> 64 with grad: features {rel_err(out, F):.2e}, gradients {['%.2e' % e for e in errs]}")
    assert rel_err(out, F) <= TOL and max(errs) <= TOL
    with pytest.raises(GaeHipError, match="128"):
        model.embed_graphs(ds, fused=True, grad=True)


def test_the_backward_kernel_refuses_what_it_cannot_hold(dev):
    """39 -> 64 -> 64 -> 64 is taken by the forward kernel and not by the backward: fused=True with a gradient raises
    naming the shape (never a detached tensor), "auto" takes the chunked route, no_grad is untouched"""
    from gae_dgl_amd import _lib, ops
    from gae_dgl_amd._lib import GaeHipError
    assert ops.embed_graphs_usable(39, [64, 64, 64]) and not ops.embed_graphs_bwd_usable(39, [64, 64, 64])
    rng = np.random.default_rng(3)
    arrays = random_set(rng, rng.integers(2, 30, 40))
    ds = make_ds(arrays, dev, "uint8")
    model = make_model([64, 64, 64], "none", dev, seed=1)
    with pytest.raises(GaeHipError, match=r"64, 64, 64"):
        model.embed_graphs(ds, fused=True, grad=True)
    lins = [l.apply_mod.linear for l in model.layers]
    with pytest.raises(GaeHipError, match=r"64, 64, 64"):
        ops.embed_graphs(ds.graph_ptr, ds.indptr, ds.indices, ds.feat, [l.weight for l in lins], [l.bias for l in lins],
                         [1, 1, 0])
    before = _lib.CALLS["gae_embed_graphs"]
    out = model.embed_graphs(ds, fused="auto", grad=True)
    assert out.requires_grad and _lib.CALLS["gae_embed_graphs"] == before
    assert torch.equal(model.embed_graphs(ds, fused=True), model.embed_graphs(ds, fused="auto"))   # no_grad: the kernel


# ------------------------------------------------------------------ 7. one training step, end to end
def test_a_linear_head_with_mse_end_to_end(zinc2000, dev):
    gp, src, dst, X = zinc2000
    keep = 200
    arrays = (gp[:keep + 1], src[src < gp[keep]], dst[dst < gp[keep]], X[:gp[keep]])
    ds = make_ds(arrays, dev, "uint8")
    model = make_model([32, 16], "none", dev, seed=12)
    torch.manual_seed(13)
    head = torch.nn.Linear(48, 1)
    y = torch.randn(keep)
    # fp64 restatement of the whole chain on the CPU
    Ws, bs = R.params_of(model)
    hw, hb = head.weight.detach().double().requires_grad_(True), head.bias.detach().double().requires_grad_(True)
    F = R.features(*arrays, Ws, bs, "none")
    loss_ref = ((F @ hw.t() + hb).squeeze(1) - y.double()).pow(2).mean()
    ref = torch.autograd.grad(loss_ref, Ws + bs + [hw, hb])
    # the product
    head = head.to(dev)
    bg = ds.batch(np.arange(keep))
    h = bg.ndata['h']; h0 = h.clone(); keys = set(bg.ndata)
    snap = [p.detach().clone() for p in model.parameters()]
    for data in (ds, bg):
        for p in list(model.parameters()) + list(head.parameters()):
            p.grad = None
        feats = model.embed_graphs(data, fused=True, grad=True)
        loss = torch.nn.functional.mse_loss(head(feats).squeeze(1), y.to(dev))
        for p, v in zip(model.parameters(), snap):
            assert torch.equal(p.detach(), v)                      # the forward touches no parameter
        assert bg.ndata['h'] is h and torch.equal(h, h0) and set(bg.ndata) == keys
        loss.backward()
        got = [p.grad for p in params_of(model)] + [head.weight.grad, head.bias.grad]
        errs = [rel_err(g, r) for g, r in zip(got, ref)]
        print(f"end to end: loss {float(loss.detach()):.6f} vs {float(loss_ref):.6f} | {['%.2e' % e for e in errs]}")
        assert abs(float(loss.detach()) - float(loss_ref)) <= TOL * max(1.0, float(loss_ref))
        assert max(errs) <= TOL


# ------------------------------------------------------------------ 8. the script
def test_finetune_script_on_a_train_inductive_checkpoint(tmp_path, dev, capsys):
    from gae_dgl_amd import finetune as FT, train_inductive as TI
    from gae_dgl_amd.dataset import DeviceGraphDataset
    TI.main(["--hidden_dims", "32", "16", "--synthetic", "600", "-b", "128", "-e", "1", "--seed", "0", "--no_plot",
             "-s", str(tmp_path)])
    ckpt = os.path.join(str(tmp_path), "ep00.pkl")
    ds = DeviceGraphDataset.synthetic_zinc(600, seed=0, device=dev)
    targets = os.path.join(str(tmp_path), "y.npy")
    np.save(targets, np.asarray(ds.sizes_host, dtype=np.float32))                  # the atom count of each molecule
    sd0 = torch.load(ckpt, map_location="cpu")
    common = ["--checkpoint", ckpt, "--hidden_dims", "32", "16", "--synthetic", "600", "--seed", "0", "--targets",
              targets, "--epochs", "3", "-b", "128", "--lr", "0.01"]
    for extra, frozen in (([], False), (["--freeze_encoder", "--head", "mlp"], True)):
        out = os.path.join(str(tmp_path), "frozen" if frozen else "tuned")
        capsys.readouterr()
        losses = FT.main(common + ["--out", out] + extra)
        printed = capsys.readouterr().out
        assert printed.count("train MSE") == 3 and "Epoch: 02" in printed
        assert len(losses) == 3 and np.isfinite(losses).all() and losses[-1] < losses[0], losses
        sd = torch.load(os.path.join(out, "encoder.pkl"), map_location="cpu")
        assert list(sd.keys()) == list(sd0.keys()) == [
            "layers.0.apply_mod.linear.weight", "layers.0.apply_mod.linear.bias",
            "layers.1.apply_mod.linear.weight", "layers.1.apply_mod.linear.bias"]
        same = [torch.equal(sd[k], sd0[k]) for k in sd]
        assert all(same) if frozen else not any(same)
        head = torch.load(os.path.join(out, "head.pkl"), map_location="cpu")
        assert len(head) == (4 if frozen else 2)
