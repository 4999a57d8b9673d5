"""The per-member reconstruction loss (GAE.reconstruction_loss(g, scope="graph"), gae_decoder_bce_graphs) on the GPU:
pinned to reference-generated fixtures, a single member equal to the batch loss, seeded fuzz against fp64, in-launch
dropout, fixed-capacity batches, repeatability, captured training and the command line."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel_err(a, b):
    a = torch.as_tensor(a).detach().double().cpu(); b = torch.as_tensor(np.asarray(b) if not torch.is_tensor(b) else b)
    b = b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp(min=1.0)) if b.numel() else 0.0


def build_model(g):
    import gae_dgl_amd as G
    model = G.GAE(g["X"].shape[1], [int(h) for h in g["hidden"]])
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd/")})
    return model.to(DEV)


def graph_of(n, src, dst, X=None, sizes=None):
    import gae_dgl_amd as G
    gr = G.DGLGraph()
    gr.add_nodes(int(n)); gr.add_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64))
    gr.to(DEV)
    if X is not None:
        gr.ndata['h'] = torch.from_numpy(np.asarray(X)).to(DEV)
    if sizes is not None:
        gr.batch_num_nodes = [int(s) for s in sizes]
    return gr


# ----------------------------------------------------------------- (a) the reference's per-molecule loss
@pytest.mark.parametrize("tag", ["p0", "p01"])
def test_mol8_matches_reference_fixture(tag):
    import gae_dgl_amd as G
    fx, whole, parts = load_golden("mol8_graph_scope"), load_golden("mol8"), load_golden("mol8_parts")
    gs = [graph_of(parts[f"g{i}/n"], parts[f"g{i}/src"], parts[f"g{i}/dst"], parts[f"g{i}/X"])
          for i in range(int(parts["n_graphs"]))]
    bg = G.batch(gs)
    assert bg.graph_ptr().cpu().tolist() == fx["node_ptr"].tolist()
    model = build_model(whole)
    model.decoder.dropout = 0.0 if tag == "p0" else 0.1
    model.decoder.mask = None if tag == "p0" else torch.from_numpy(whole["mask"]).to(DEV)
    loss = model.reconstruction_loss(bg, scope="graph")
    assert rel_err(loss, fx["loss_" + tag]) < TOL
    loss.backward()
    for k, p in model.named_parameters():
        assert rel_err(p.grad, fx[f"grad_{tag}/{k}"]) < TOL, k
    # the per-member losses of the same launch
    from gae_dgl_amd import ops
    bg.ndata['h'] = torch.from_numpy(whole["X"]).to(DEV)        # (the loss left the embedding there, gae.py:53)
    z = model.encode(bg).detach()
    _, gl = ops.decoder_bce_graphs(z, model.decoder.mask, bg, graph_loss=True)
    assert rel_err(gl, fx["graph_loss_" + tag]) < TOL


# ----------------------------------------------------------------- (b) one member: exactly the batch loss
@pytest.mark.parametrize("name", ["tiny", "single", "deep3", "sym200", "wide300", "wide2k"])
def test_single_member_equals_reference_batch_loss(name):
    g = load_golden(name)
    for tag, mask in (("p0", None), ("p01", g.get("mask"))):
        if "loss_" + tag not in g or (tag == "p01" and mask is None):
            continue
        model = build_model(g)
        model.decoder.dropout = 0.0 if mask is None else 0.1
        model.decoder.mask = None if mask is None else torch.from_numpy(mask).to(DEV)
        gr = graph_of(g["n"], g["src"], g["dst"], g["X"])
        loss = model.reconstruction_loss(gr, scope="graph")
        assert rel_err(loss, g["loss_" + tag]) < TOL, tag
        loss.backward()
        for k, p in model.named_parameters():
            assert rel_err(p.grad, g[f"grad_{tag}/{k}"]) < TOL, (tag, k)


# ----------------------------------------------------------------- (c) seeded fuzz against fp64
def fp64_graph_scope(Zt, node_ptr, src, dst, window=2048):
    """(loss, per-member losses, dZt) in fp64 on the device, windowed over rows (large members)"""
    Zt = Zt.double()
    dZ = torch.zeros_like(Zt)
    src = torch.as_tensor(src, device=DEV); dst = torch.as_tensor(dst, device=DEV)
    ptr = [int(v) for v in node_ptr]
    members = []
    for g in range(len(ptr) - 1):
        p0, p1 = ptr[g], ptr[g + 1]
        n = p1 - p0
        inside = (src >= p0) & (src < p1) & (dst >= p0) & (dst < p1)
        s_, d_ = src[inside] - p0, dst[inside] - p0
        S = int(inside.sum())
        if n == 0 or S == 0:
            members.append(None)
            continue
        pw = (n * n - S) / S
        Zg = Zt[p0:p1]
        tot = 0.0
        rows_g = []
        for r0 in range(0, n, window):
            r1 = min(n, r0 + window)
            x = Zg[r0:r1] @ Zg.T
            y = torch.zeros(r1 - r0, n, dtype=torch.float64, device=DEV)
            yt = torch.zeros_like(y)
            sel = (d_ >= r0) & (d_ < r1)
            y.index_put_((d_[sel] - r0, s_[sel]), torch.ones(int(sel.sum()), dtype=torch.float64, device=DEV), accumulate=True)
            sel = (s_ >= r0) & (s_ < r1)
            yt.index_put_((s_[sel] - r0, d_[sel]), torch.ones(int(sel.sum()), dtype=torch.float64, device=DEV), accumulate=True)
            tot += float(((1 - y) * x + (1 + (pw - 1) * y) * torch.nn.functional.softplus(-x)).sum())
            c = (1 - y) - (1 + (pw - 1) * y) * torch.sigmoid(-x) + (1 - yt) - (1 + (pw - 1) * yt) * torch.sigmoid(-x)
            rows_g.append((r0, r1, (c @ Zg) / (n * n)))
        members.append(tot / (n * n))
        for r0, r1, v in rows_g:
            dZ[p0 + r0:p0 + r1] = v
        members[-1] = (members[-1], (p0, p1))
    valid = [m for m in members if m is not None]
    Gp = len(valid)
    loss = sum(m[0] for m in valid) / Gp if Gp else float("nan")
    if Gp:
        dZ /= Gp
    per = [float("nan") if m is None else m[0] for m in members]
    return loss, per, dZ


def fuzz_batch(rng, sizes, extra_edges=()):
    """molecule-like members (a chain plus random chords, both directions), some without any edge"""
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    src, dst = [], []
    for g, n in enumerate(sizes):
        if n < 2 or rng.random() < 0.08:
            continue                                   # a member with no edges
        a = np.arange(n - 1); b = a + 1
        k = max(1, n // 4)
        ca, cb = rng.integers(0, n, k), rng.integers(0, n, k)
        s = np.concatenate([a, b, ca]); d = np.concatenate([b, a, cb])
        if rng.random() < 0.5:
            keep = rng.random(len(s)) > 0.15           # some directed members
            s, d = s[keep], d[keep]
        src.append(s + ptr[g]); dst.append(d + ptr[g])
    src = np.concatenate(src) if src else np.zeros(0, np.int64)
    dst = np.concatenate(dst) if dst else np.zeros(0, np.int64)
    if len(src) > 2:                                   # a repeated edge
        src = np.concatenate([src, src[:2]]); dst = np.concatenate([dst, dst[:2]])
    for s, d in extra_edges:
        src = np.append(src, s); dst = np.append(dst, d)
    return ptr, src.astype(np.int64), dst.astype(np.int64)


FUZZ = [  # (seed, member sizes, d)
    (1, "mixed60", 16), (2, "small600", 3), (3, "mixed60", 33), (4, "mixed60", 1), (5, "mixed60", 64),
    (6, "huge", 16),
]


@pytest.mark.parametrize("seed,kind,d", FUZZ)
def test_fuzz_against_fp64(seed, kind, d):
    from gae_dgl_amd import ops
    rng = np.random.default_rng(seed)
    if kind == "mixed60":
        sizes = rng.integers(1, 301, 60); sizes[3] = 90; sizes[7] = 280; sizes[11] = 0; sizes[12] = 1
    elif kind == "small600":
        sizes = rng.integers(1, 41, 600)
    else:
        sizes = np.concatenate([rng.integers(9, 39, 2000), [20000], rng.integers(9, 39, 2000)])
    ptr, src, dst = fuzz_batch(rng, sizes)
    # an edge that leaves its member (ignored by the loss)
    a, b = int(ptr[1]), int(ptr[-2])
    src = np.append(src, a); dst = np.append(dst, b)
    n = int(ptr[-1])
    gr = graph_of(n, src, dst, sizes=sizes)
    Z = (torch.randn(n, d, generator=torch.Generator().manual_seed(seed)) * 0.6).to(DEV).requires_grad_()
    loss, gl = ops.decoder_bce_graphs(Z, None, gr, graph_loss=True)
    ops.backward(loss)
    ref_loss, ref_gl, ref_dZ = fp64_graph_scope(Z.detach(), ptr, src, dst)
    assert abs(float(loss.detach()) - ref_loss) < TOL * max(1.0, abs(ref_loss))
    gl = gl.cpu().numpy().astype(np.float64)
    ref_gl = np.asarray(ref_gl)
    assert np.array_equal(np.isnan(gl), np.isnan(ref_gl))
    ok = ~np.isnan(ref_gl)
    assert np.abs(gl[ok] - ref_gl[ok]).max() < TOL * max(1.0, np.abs(ref_gl[ok]).max())
    # relative to the gradient's own scale (it is 1 / (G' n_g^2) small)
    scale = float(ref_dZ.abs().max())
    assert float((Z.grad.double() - ref_dZ).abs().max()) <= 1e-5 * scale


def test_no_member_counts_gives_nan():
    from gae_dgl_amd import ops
    gr = graph_of(10, [], [], sizes=[4, 6])
    Z = torch.randn(10, 8, device=DEV, requires_grad=True)
    loss, gl = ops.decoder_bce_graphs(Z, None, gr, graph_loss=True)
    ops.backward(loss)
    assert np.isnan(float(loss.detach())) and bool(torch.isnan(gl).all())
    assert float(Z.grad.abs().max()) == 0.0


# ----------------------------------------------------------------- (d) dropout drawn in the launch
def test_dropout_in_launch_matches_dropout_mask():
    from gae_dgl_amd import ops
    rng = np.random.default_rng(9)
    sizes = rng.integers(5, 40, 50)
    ptr, src, dst = fuzz_batch(rng, sizes)
    n, d = int(ptr[-1]), 16
    gr = graph_of(n, src, dst, sizes=sizes)
    Z = torch.randn(n, d, device=DEV)
    draws = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    mask = torch.empty(n, d, device=DEV)
    loss = ops.decoder_bce_graphs(Z, mask, gr, dropout=(0.1, 1234, 0, draws))
    torch.cuda.synchronize()
    assert int(draws) == 6
    want = ops.dropout_mask((n, d), 0.1, 1234, 0, DEV, draw_counter=torch.full((1,), 5, dtype=torch.int64, device=DEV))
    assert torch.equal(mask, want)
    again = ops.decoder_bce_graphs(Z, want, gr)              # the same mask given as an input
    assert float(loss) == float(again)


# ----------------------------------------------------------------- (e) fixed-capacity batch
def test_padded_batch_equals_unpadded():
    from gae_dgl_amd import ops
    rng = np.random.default_rng(21)
    sizes = rng.integers(9, 39, 200)
    ptr, src, dst = fuzz_batch(rng, sizes)
    n, d = int(ptr[-1]), 16
    Z = torch.randn(n + 77, d, device=DEV)
    plain = graph_of(n, src, dst, sizes=sizes)
    z0 = Z[:n].clone().requires_grad_()
    l0 = ops.decoder_bce_graphs(z0, None, plain)
    ops.backward(l0)
    padded = graph_of(n + 77, src, dst, sizes=list(sizes))
    counts = torch.tensor([n, len(src), 0, 0], dtype=torch.int64, device=DEV)
    z1 = Z.clone().requires_grad_()
    l1 = ops.decoder_bce_graphs(z1, None, padded, counts=counts)
    ops.backward(l1)
    assert float(l0.detach()) == float(l1.detach())
    assert torch.equal(z1.grad[:n], z0.grad)
    assert float(z1.grad[n:].abs().max()) == 0.0
    # a member that ends behind counts[0] is left out: the loss of the batch without it
    cut = int(ptr[-2])
    counts2 = torch.tensor([cut, 0, 0, 0], dtype=torch.int64, device=DEV)
    z2 = Z.clone().requires_grad_()
    l2, gl2 = ops.decoder_bce_graphs(z2, None, padded, counts=counts2, graph_loss=True)
    ops.backward(l2)
    keep = src < cut
    short = graph_of(cut, src[keep], dst[keep], sizes=sizes[:-1])
    z3 = Z[:cut].clone().requires_grad_()
    l3 = ops.decoder_bce_graphs(z3, None, short)
    ops.backward(l3)
    assert float(l2.detach()) == float(l3.detach()) and bool(torch.isnan(gl2[-1]))
    assert torch.equal(z2.grad[:cut], z3.grad) and float(z2.grad[cut:].abs().max()) == 0.0


# ----------------------------------------------------------------- (f) repeatability, validation mode
def test_repeatable_and_loss_only():
    from gae_dgl_amd import ops
    rng = np.random.default_rng(33)
    sizes = np.concatenate([rng.integers(1, 300, 40), [150, 70]])
    ptr, src, dst = fuzz_batch(rng, sizes)
    n = int(ptr[-1])
    gr = graph_of(n, src, dst, sizes=sizes)
    Z = torch.randn(n, 16, device=DEV)
    runs = []
    for _ in range(2):
        z = Z.clone().requires_grad_()
        loss, gl = ops.decoder_bce_graphs(z, None, gr, graph_loss=True)
        ops.backward(loss)
        runs.append((loss.detach().clone(), gl.clone(), z.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2])
    assert torch.equal(torch.nan_to_num(runs[0][1], nan=-1.0), torch.nan_to_num(runs[1][1], nan=-1.0))
    with torch.no_grad():
        l_only = ops.decoder_bce_graphs(Z, None, gr)         # dZ = NULL
    assert torch.equal(l_only.reshape(1), runs[0][0].reshape(1))


# ----------------------------------------------------------------- (g) captured training
def test_captured_training_matches_eager():
    import gae_dgl_amd as G
    from gae_dgl_amd import ops, workloads as W
    from gae_dgl_amd.capture import CapturedInductiveStep
    from gae_dgl_amd.dataset import DeviceGraphDataset
    from gae_dgl_amd.optim import Adam
    gp, s, d, X = W.zinc_like(300, seed=11)
    ds = DeviceGraphDataset(gp, s, d, X, device=DEV)
    B = 32
    torch.manual_seed(3)
    m_e = G.GAE(ds.n_feat, [32, 16]).to(DEV)
    m_e.decoder.seed = 77
    m_c = copy.deepcopy(m_e)
    o_e, o_c = Adam(m_e.parameters(), lr=1e-2), Adam(m_c.parameters(), lr=1e-2)
    rng = np.random.default_rng(0)
    orders = [rng.permutation(ds.ids) for _ in range(2)]
    runner = CapturedInductiveStep(m_c, o_c, ds, B, loss_scope="graph")
    losses_c = [float(loss) for order in orders for loss in runner.epoch(order)]
    losses_e = []
    for order in orders:
        d_order = torch.from_numpy(order).to(DEV)
        for lo in range(0, len(order), B):
            bg = ds._assemble(d_order[lo:lo + B], order[lo:lo + B])
            o_e.zero_grad()
            loss = m_e.reconstruction_loss(bg, scope="graph")
            ops.backward(loss)
            o_e.step()
            losses_e.append(float(loss))
    assert len(losses_c) == len(losses_e) == 2 * ((300 + B - 1) // B)
    np.testing.assert_allclose(losses_c, losses_e, rtol=1e-5)
    for pc, pe in zip(m_c.parameters(), m_e.parameters()):
        assert float((pc - pe).abs().max()) <= 1e-5 * max(float(pe.abs().max()), 1e-3) + 2e-6
    # and it is not the batch-scope loss
    bg = ds._assemble(torch.from_numpy(orders[0][:B]).to(DEV), orders[0][:B])
    m_e.decoder.dropout = 0.0
    with torch.no_grad():
        a = float(m_e.reconstruction_loss(bg, scope="graph"))
        bg = ds._assemble(torch.from_numpy(orders[0][:B]).to(DEV), orders[0][:B])
        b = float(m_e.reconstruction_loss(bg))
    assert abs(a - b) > 1e-3 * abs(b)


# ----------------------------------------------------------------- (h) command line
def test_cli_graph_scope_epoch(tmp_path):
    out = tmp_path / "run"
    r = subprocess.run([sys.executable, "-m", "gae_dgl_amd.train_inductive", "--synthetic", "2000", "--loss_scope",
                        "graph", "-e", "1", "--hidden_dims", "32", "16", "--save_dir", str(out), "--no_plot",
                        "--seed", "0"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (out / "ep00.pkl").exists()
    assert "Epoch: 00" in r.stdout
