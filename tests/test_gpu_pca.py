"""K31 on the device (gae_pca_solve / gae_pca_transform, ops.pca): the bits of tests/pca_ref.py from the device's own
moments, the derived projection bound, determinism, the failure paths and the wrappers."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import pca_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ptr(t):
    import ctypes
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def device_solve(X, rows, k, *, ldx=None, stream=None):
    """(stats, pivot, mean, values, components, status words) through the C ABI: gae_ridge_stats as ops.pca calls it
    (folds = 1, t = 1, Y = column 0 of X), then gae_pca_solve"""
    from gae_dgl_amd import _lib
    n, d = X.shape
    Xd = torch.from_numpy(X).to(DEV)
    if ldx is not None:
        wide = torch.full((n, ldx), float("nan"), device=DEV)
        wide[:, :d] = Xd
        Xd = wide[:, :d]
    listed = None if rows is None else torch.from_numpy(np.asarray(rows)).to(DEV).to(torch.int32)
    n_used = n if listed is None else listed.shape[0]
    px = (Xd if listed is None else Xd.index_select(0, listed.long())).mean(0)
    piv = torch.cat([px, px[:1]]).contiguous()
    W = d + 2
    lib = _lib.load()
    ws = torch.empty(max(lib.gae_ridge_workspace_bytes(n_used, d, 1, 1), lib.gae_pca_workspace_bytes(d)), dtype=torch.uint8, device=DEV)
    fold_ptr = torch.tensor([0, n_used], dtype=torch.int32, device=DEV)
    stats = torch.empty(W * (W + 1) // 2, dtype=torch.float64, device=DEV)
    rstatus = torch.zeros(4, dtype=torch.int64, device=DEV)
    status = torch.zeros(8, dtype=torch.int64, device=DEV)
    mean = torch.empty(d, dtype=torch.float64, device=DEV)
    values = torch.empty(k, dtype=torch.float64, device=DEV)
    comps = torch.empty(k, d, dtype=torch.float64, device=DEV)
    s = torch.cuda.current_stream() if stream is None else stream
    with torch.cuda.stream(s):
        h = ctypes_stream(s)
        _lib.call("gae_ridge_stats", _ptr(Xd), Xd.stride(0), _ptr(Xd), Xd.stride(0), n, d, 1, _ptr(piv), _ptr(listed), n_used,
                  _ptr(fold_ptr), 1, _ptr(stats), _ptr(rstatus), _ptr(ws), ws.numel(), h)
        _lib.call("gae_pca_solve", _ptr(stats), d, 1, _ptr(piv), n_used, k, 0, _ptr(mean), _ptr(values), _ptr(comps),
                  _ptr(status), _ptr(ws), ws.numel(), h)
    s.synchronize()
    assert rstatus.tolist() == [0, 0, 0, 0]
    return (stats.cpu().numpy(), piv.cpu().numpy(), mean.cpu().numpy(), values.cpu().numpy(), comps.cpu().numpy(),
            status.cpu().numpy())


def ctypes_stream(s):
    import ctypes
    return ctypes.c_void_p(s.cuda_stream)


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(X, rows, k, device outputs, restatement on the device's own stats), computed once and shared"""
    case = next(c for c in R.CASES if c[0] == name)
    X, rows, k = R.make(case)
    out = device_solve(X, rows, k)
    ref = R.solve(out[0], X.shape[1], 1, out[1], k)
    return X, rows, k, out, ref


@pytest.mark.parametrize("name", [c[0] for c in R.CASES])
def test_solve_and_transform_bit_for_bit(name):
    """gae_pca_solve on the device's own stats gives exactly pca_ref.solve's mean, values, components and sweep count;
    gae_pca_transform exactly pca_ref.transform's scores, plain and whitened"""
    from gae_dgl_amd import ops
    X, rows, k, (stats, piv, mean, values, comps, status), ref = case_data(name)
    info, sweeps, rotations = int(status[0]), int(status[1]), int(status[2])
    off, total = status[6:8].view(np.float64)
    print(f"{name}: info {info} sweeps {sweeps} (ref {ref.n_sweeps}) rotations {rotations} (ref {ref.n_rotations}) "
          f"off {off:.3e} (ref {ref.off_norm:.3e})")
    assert (info, sweeps, rotations) == (ref.info, ref.n_sweeps, ref.n_rotations) and info == 0
    assert np.array_equal(mean, ref.mean)
    assert np.array_equal(values, ref.values)
    assert np.array_equal(comps, ref.components)
    assert off == ref.off_norm and total == ref.total_variance
    Xd = torch.from_numpy(X).to(DEV)
    rd = None if rows is None else torch.from_numpy(rows).to(DEV)
    md, cd, vd = (torch.from_numpy(a).to(DEV) for a in (mean, comps, values))
    for whiten in (False, True):
        st = torch.zeros(8, dtype=torch.int64, device=DEV)
        Z = ops.pca_transform(Xd, md, cd, vd, whiten, rows=rd, status=st).cpu().numpy()
        Zr = R.transform(X, mean, comps, values, whiten, rows)
        assert Z.shape == Zr.shape and np.array_equal(Z, Zr), (name, whiten, np.abs(Z - Zr).max())
        assert st.tolist()[3] == 0 and st.tolist()[5] == 0
        assert st.tolist()[4] == (int((values <= 0).sum()) if whiten else 0)


@pytest.mark.parametrize("name", ["d3", "d17", "d48", "d128", "bigmean", "subset"])
def test_projection_error_is_inside_the_fma_chain_bound(name):
    """|Z - Z64| <= (d + 2) 2^-24 sum_j |x_ij - m_j| |v_cj|, the fma-chain bound: one rounding of the difference and one
    of v_cj (2 2^-24 on a term, to first order) and the d roundings of a chain of d fused steps -- d + 2 in all.  m is
    the mean the kernel is stated to use, rounded to fp32 once: that rounding is no part of the chain and is not
    relative to x - m (the "bigmean" case: |m| = 1e4 beside a unit spread measured 36 x this bound against the
    unrounded mean), so Z64 is taken about the fp32 mean here; against the fp64 mean the same bound holds with the
    rounding's own term 2^-24 sum_j |m_j| |v_cj| added, which is asserted too"""
    X, rows, k, (stats, piv, mean, values, comps, status), ref = case_data(name)
    from gae_dgl_amd import ops
    Xd = torch.from_numpy(X).to(DEV)
    rd = None if rows is None else torch.from_numpy(rows).to(DEV)
    Z = ops.pca_transform(Xd, torch.from_numpy(mean).to(DEV), torch.from_numpy(comps).to(DEV), rows=rd).cpu().numpy()
    Xl = (X if rows is None else X[rows]).astype(np.float64)
    m32 = mean.astype(np.float32).astype(np.float64)
    Z64 = (Xl - m32) @ comps.T
    bound = (X.shape[1] + 2) * 2.0 ** -24 * (np.abs(Xl - m32) @ np.abs(comps.T))
    print(f"{name}: worst error / bound {np.max(np.abs(Z - Z64) / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(np.abs(Z - Z64) <= bound)
    exact = (Xl - mean) @ comps.T
    wider = (X.shape[1] + 2) * 2.0 ** -24 * (np.abs(Xl - mean) @ np.abs(comps.T)) + 2.0 ** -24 * (np.abs(mean) @ np.abs(comps.T))
    print(f"{name}: against the fp64 mean, worst error / bound {np.max(np.abs(Z - exact) / np.maximum(wider, 1e-300)):.3f}")
    assert np.all(np.abs(Z - exact) <= wider)


def test_ops_pca_against_the_direct_answer_and_its_fields():
    from gae_dgl_amd import ops
    X, rows, k, (stats, piv, mean, values, comps, status), ref = case_data("d48")
    Xd = torch.from_numpy(X).to(DEV)
    res = ops.pca(Xd, 5)
    full = R.solve(stats, 48, 1, piv, 48)
    assert np.array_equal(res.components.cpu().numpy(), full.components[:5])
    assert np.array_equal(res.explained_variance.cpu().numpy(), full.values[:5])
    assert np.array_equal(res.mean.cpu().numpy(), full.mean)
    assert (res.n_used, res.n_sweeps, res.info) == (1000, full.n_sweeps, 0)
    assert np.array_equal(res.explained_variance_ratio.cpu().numpy(), full.values[:5] / full.total_variance)
    assert np.array_equal(res.singular_values.cpu().numpy(), np.sqrt(full.values[:5] * 999.0))
    m, C, w, V = R.direct(X)
    assert np.allclose(res.explained_variance.cpu().numpy(), w[:5], rtol=1e-12, atol=0)
    assert np.abs(np.abs(res.components.cpu().numpy() @ V[:5].T) - np.eye(5)).max() < 1e-9
    Z = res.transform(Xd)
    assert np.array_equal(Z.cpu().numpy(), R.transform(X, full.mean, full.components[:5]))
    back = res.inverse_transform(ops.pca(Xd).transform(Xd)[:, :5])
    assert back.dtype == torch.float64 and back.shape == (1000, 48)
    allc = ops.pca(Xd)
    assert float((allc.inverse_transform(allc.transform(Xd)) - Xd.double()).abs().max()) < 1e-4
    # a bool mask lists the same rows as its ids; whiten only changes transform
    Xs, rs, _ = R.make(next(c for c in R.CASES if c[0] == "subset"))
    Xsd = torch.from_numpy(Xs).to(DEV)
    mask = torch.zeros(Xs.shape[0], dtype=torch.bool, device=DEV)
    mask[torch.from_numpy(rs).to(DEV)] = True
    a, b = ops.pca(Xsd, 2, rows=torch.from_numpy(rs).to(DEV)), ops.pca(Xsd, 2, rows=mask, whiten=True)
    assert torch.equal(a.components, b.components) and torch.equal(a.explained_variance, b.explained_variance)
    assert a.n_used == b.n_used == len(rs)
    Zw = b.transform(Xsd, rows=mask).cpu().numpy()
    assert np.array_equal(Zw, R.transform(Xs, b.mean.cpu().numpy(), b.components.cpu().numpy(),
                                          b.explained_variance.cpu().numpy(), True, rs))
    assert abs(float(np.var(Zw[:, 0].astype(np.float64), ddof=1)) - 1.0) < 1e-5


def test_same_bits_run_to_run_for_any_ldx_and_stream():
    from gae_dgl_amd import ops
    X, rows, k, base, ref = case_data("d17")
    again = device_solve(X, rows, k)
    wide = device_solve(X, rows, k, ldx=29)
    side = device_solve(X, rows, k, stream=torch.cuda.Stream(device=DEV))
    for other in (again, wide, side):
        for a, b in zip(base, other):
            assert np.array_equal(a, b)
    Xd = torch.from_numpy(X).to(DEV)
    first = ops.pca(Xd, 3)
    Z0 = first.transform(Xd)
    ops.tsne(Xd, n_iter=2, perplexity=5.0)                                  # another workspace user in between
    ops.tsne(Xd, n_iter=0, init="pca")
    second = ops.pca(Xd, 3)
    assert torch.equal(first.components, second.components) and torch.equal(first.explained_variance, second.explained_variance)
    assert torch.equal(Z0, second.transform(Xd))
    padded = torch.zeros(X.shape[0], 40, device=DEV)
    padded[:, :17] = Xd
    assert torch.equal(Z0, first.transform(padded[:, :17]))


def test_failure_paths():
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    X, rows, k, out, ref = case_data("d16")
    Xd = torch.from_numpy(X).to(DEV)
    bad = Xd.clone()
    bad[100, 3] = float("nan")
    with pytest.raises(GaeHipError, match="non-finite"):
        ops.pca(bad)
    keep = torch.ones(X.shape[0], dtype=torch.bool, device=DEV)
    keep[100] = False
    assert ops.pca(bad, 2, rows=keep).info == 0                              # the poisoned row is not listed: never read
    with pytest.raises(GaeHipError):
        ops.pca(Xd, 17)
    with pytest.raises(GaeHipError):
        ops.pca(torch.zeros(10, 129, device=DEV))
    with pytest.raises(ValueError):
        ops.pca(Xd[:1])
    with pytest.raises(ValueError):
        ops.pca(Xd, rows=torch.tensor([5], device=DEV))
    with pytest.raises(GaeHipError):
        ops.pca(torch.from_numpy(X))
    # a poisoned listed row of transform: a NaN row, counted; the others keep their bits
    res = ops.pca(Xd, 2)
    st = torch.zeros(8, dtype=torch.int64, device=DEV)
    Zb = ops.pca_transform(bad, res.mean, res.components, status=st)
    Z = res.transform(Xd)
    assert bool(torch.isnan(Zb[100]).all()) and st.tolist()[3] == 1
    ok = torch.arange(X.shape[0], device=DEV) != 100
    assert torch.equal(Zb[ok], Z[ok])
    # whitening a component without variance gives 0 and is counted
    Xc, _, _ = R.make(next(c for c in R.CASES if c[0] == "constcol"))
    Xcd = torch.from_numpy(Xc).to(DEV)
    full = ops.pca(Xcd, whiten=True)
    lam = full.explained_variance.clone()
    lam[-1] = 0.0
    st = torch.zeros(8, dtype=torch.int64, device=DEV)
    Zw = ops.pca_transform(Xcd, full.mean, full.components, lam, True, status=st)
    assert float(Zw[:, -1].abs().max()) == 0.0 and st.tolist()[4] == 1 and bool(torch.isfinite(Zw).all())
    # gae_pca_solve on moments of fewer than two rows: info -1, NaN outputs
    one = device_solve_raw_one_row()
    assert one[0] == -1 and np.isnan(one[1]).all() and np.isnan(one[2]).all()


def device_solve_raw_one_row():
    from gae_dgl_amd import _lib
    d, W = 3, 5
    stats = torch.from_numpy(R.moments(np.array([[1.0, 2.0, 3.0]], np.float32))).to(DEV)
    status = torch.zeros(8, dtype=torch.int64, device=DEV)
    mean, values, comps = (torch.zeros(s, dtype=torch.float64, device=DEV) for s in (3, 2, 6))
    ws = torch.empty(_lib.load().gae_pca_workspace_bytes(d), dtype=torch.uint8, device=DEV)
    _lib.call("gae_pca_solve", _ptr(stats), d, 1, None, 1, 2, 0, _ptr(mean), _ptr(values), _ptr(comps), _ptr(status), _ptr(ws),
              ws.numel(), ctypes_stream(torch.cuda.current_stream()))
    torch.cuda.synchronize()
    return int(status[0]), values.cpu().numpy(), comps.cpu().numpy()


# ------------------------------------------------------------------------------------------------ wrappers and CLIs
def test_tsne_init_pca_starts_from_the_stated_map_and_leaves_the_others_alone():
    """iteration 0 (n_iter = 0 returns the start): the first two scores times the fp32 rounding of 1e-4 / sigma, sigma =
    sqrt(lambda_1 (n - 1) / n); d = 1: the second coordinate is zero; init=None and init=<tensor> keep their bits"""
    from gae_dgl_amd import ops
    X, rows, k, (stats, piv, mean, values, comps, status), ref = case_data("d17")
    n = X.shape[0]
    Xd = torch.from_numpy(X).to(DEV)
    Y0 = ops.tsne(Xd, n_iter=0, init="pca").embedding.cpu().numpy()
    scale = np.float32(1e-4 / np.sqrt(ref.values[0] * (n - 1) / n))
    want = R.transform(X, ref.mean, ref.components[:2]) * scale
    assert Y0.dtype == np.float32 and np.array_equal(Y0, want)
    assert abs(float(np.std(Y0[:, 0].astype(np.float64))) - 1e-4) < 1e-9
    X1, _, _ = R.make(next(c for c in R.CASES if c[0] == "d2n1000"))
    one = torch.from_numpy(X1[:300, :1].copy()).to(DEV)
    Y1 = ops.tsne(one, n_iter=0, init="pca").embedding
    assert float(Y1[:, 1].abs().max()) == 0.0 and abs(float(Y1[:, 0].double().std(unbiased=False)) - 1e-4) < 1e-9
    assert torch.equal(ops.tsne(Xd, n_iter=0, seed=3).embedding, ops.tsne_init(n, 3, DEV))
    given = torch.randn(n, 2, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0)) * 1e-4
    assert torch.equal(ops.tsne(Xd, n_iter=0, init=given).embedding, given)
    kw = dict(n_iter=12, perplexity=8.0, check_every=4)
    a = ops.tsne(Xd, seed=1, **kw).embedding
    ops.pca(Xd, 2)
    assert torch.equal(a, ops.tsne(Xd, seed=1, **kw).embedding)
    b = ops.tsne(Xd, init="pca", **kw).embedding
    assert bool(torch.isfinite(b).all()) and torch.equal(b, ops.tsne(Xd, init="pca", **kw).embedding) and not torch.equal(a, b)
    with pytest.raises(ValueError):
        ops.tsne(Xd, n_iter=0, init="svd")


def _golden_model(name):
    from conftest import load_golden
    import gae_dgl_amd as G
    g = load_golden(name)
    model = G.GAE(g["X"].shape[1], [int(h) for h in g["hidden"]])
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd/")})
    return g, model.to(DEV).eval()


def _graph(g):
    import gae_dgl_amd as G
    gr = G.DGLGraph()
    gr.add_nodes(int(g["n"]))
    gr.add_edges(g["src"], g["dst"])
    gr.to(torch.device(DEV))
    gr.ndata['h'] = torch.from_numpy(g["X"]).to(DEV)
    return gr


def test_pca_nodes_and_pca_graphs_agree_with_ops_pca():
    from gae_dgl_amd import ops
    from gae_dgl_amd.dataset import DeviceGraphDataset
    from gae_dgl_amd.vgae import VGAE
    from conftest import load_golden
    whole, model = _golden_model("mol8")
    gr = _graph(whole)
    feat = gr.ndata['h']
    res = model.pca_nodes(gr, 2, whiten=True)
    assert gr.ndata['h'] is feat
    with torch.no_grad():
        z = model.encode(_graph(whole))
    want = ops.pca(z, 2)
    assert torch.equal(res.components, want.components) and torch.equal(res.explained_variance, want.explained_variance)
    assert res.whiten and res.components.shape == (2, z.shape[1])
    torch.manual_seed(0)
    vg = VGAE(whole["X"].shape[1], [8, 4]).to(DEV)
    gr = _graph(whole)
    feat = gr.ndata['h']
    res = vg.pca_nodes(gr)
    assert gr.ndata['h'] is feat
    with torch.no_grad():
        mu = vg.encode(_graph(whole))[0]
    assert torch.equal(res.components, ops.pca(mu).components) and res.components.shape == (4, 4)
    parts = load_golden("mol8_parts")
    ng = int(parts["n_graphs"])
    gp = np.zeros(ng + 1, np.int64)
    np.cumsum([int(parts[f"g{i}/n"]) for i in range(ng)], out=gp[1:])
    ds = DeviceGraphDataset(gp, np.concatenate([parts[f"g{i}/src"] + gp[i] for i in range(ng)]),
                            np.concatenate([parts[f"g{i}/dst"] + gp[i] for i in range(ng)]),
                            np.concatenate([parts[f"g{i}/X"] for i in range(ng)]), device=torch.device(DEV))
    res = model.pca_graphs(ds, 3, fused="auto")
    want = ops.pca(model.embed_graphs(ds), 3)
    assert torch.equal(res.components, want.components) and torch.equal(res.mean, want.mean) and res.n_used == ng
    with pytest.raises(ValueError):
        model.pca_graphs(ds, 3, grad=True)


def test_cli_embed_pca(tmp_path, capsys):
    from gae_dgl_amd import embed as E
    import gae_dgl_amd as G
    torch.manual_seed(0)
    ckpt = str(tmp_path / "m.pkl")
    torch.save(G.GAE(39, [32, 16]).state_dict(), ckpt)
    E.main(["--checkpoint", ckpt, "--hidden_dims", "32", "16", "--synthetic", "300", "--out", str(tmp_path / "f.npy"),
            "--pca", "3", "--pca_whiten", "--pca_out", str(tmp_path / "pca.npz"),
            "--map_out", str(tmp_path / "map.npz"), "--map_iters", "10", "--map_init", "pca"])
    text = capsys.readouterr().out
    line = [l for l in text.splitlines() if l.startswith("PCA (3 of 48 components) explained variance: ")]
    assert len(line) == 1 and "(cumulative " in line[0], text
    z = np.load(tmp_path / "pca.npz")
    res = E.main.pca
    assert sorted(z.files) == ["components", "explained_variance", "explained_variance_ratio", "mean", "scores"]
    assert z["components"].shape == (3, 48) and z["components"].dtype == np.float64 and z["scores"].shape == (300, 3)
    assert np.array_equal(z["components"], res.components.cpu().numpy()) and np.array_equal(z["mean"], res.mean.cpu().numpy())
    assert np.array_equal(z["scores"], res.transform(E.main.features).cpu().numpy()) and z["scores"].dtype == np.float32
    ratio = z["explained_variance_ratio"]
    assert line[0].endswith(f"{' '.join(f'{v:.4f}' for v in ratio)} (cumulative {float(ratio.sum()):.4f})")
    assert np.allclose(z["scores"].astype(np.float64).var(0, ddof=1), 1.0, atol=1e-4)        # whitened
    from gae_dgl_amd import ops
    assert torch.equal(E.main.map.embedding, ops.tsne(E.main.features, perplexity=20.0, n_iter=10, seed=0, init="pca").embedding)
    for bad in (["--pca_out", "x.npz"], ["--pca", "49"], ["--pca", "0"], ["--map_init", "pca"]):
        with pytest.raises(SystemExit):
            E.parse_args(["--checkpoint", ckpt, "--hidden_dims", "32", "16", "--synthetic", "10", "--out", "f.npy"] + bad)


def test_cli_train_transductive_pca(tmp_path, capsys):
    from gae_dgl_amd import train_transductive as TT
    n, k = 300, 3
    rng = np.random.default_rng(0)
    comm = rng.integers(0, k, n)
    a, b = rng.integers(0, n, 6000), rng.integers(0, n, 6000)
    keep = (comm[a] == comm[b]) & (a != b)
    a, b = a[keep], b[keep]
    feats = np.eye(k, dtype=np.float32)[comm] + 0.5 * rng.standard_normal((n, k)).astype(np.float32)
    os.makedirs(tmp_path / "data", exist_ok=True)
    np.savez(tmp_path / "data" / "cora.npz", src=np.concatenate([a, b]), dst=np.concatenate([b, a]), features=feats, n=n,
             labels=comm)
    out = tmp_path / "pca.npz"
    TT.main(["--dataset", "cora", "--data_root", str(tmp_path / "data"), "-e", "10", "-s", str(tmp_path), "--seed", "0",
             "--log_every", "1000", "--pca", "2", "--pca_out", str(out)])
    text = capsys.readouterr().out
    line = [l for l in text.splitlines() if l.startswith("PCA (2 of 16 components) explained variance: ")]
    assert len(line) == 1 and "(cumulative " in line[0], text
    z = np.load(out)
    res = TT.main.last_pca
    assert z["components"].shape == (2, 16) and z["scores"].shape == (n, 2) and np.isfinite(z["scores"]).all()
    assert np.array_equal(z["components"], res.components.cpu().numpy())
    assert np.array_equal(z["explained_variance"], res.explained_variance.cpu().numpy())
    for bad in (["--pca_out", "x.npz"], ["--pca", "17"], ["--map_init", "pca"]):
        with pytest.raises(SystemExit):
            TT.parse_args(["--dataset", "cora"] + bad)
