"""K23 on the device (gae_kmeans_*, ops.kmeans / kmeans_assign / kmeans_init_pp, GAE.cluster_nodes, the two scripts)
against the fp64 restatement tests/kmeans_ref.py.  Shapes are the smallest at which each mechanism can break: one panel
and panel tails, every DH form of the product tile (d <= 16, <= 32, <= 64), one and several centre tiles and their tails,
the short and the long form of the partial-sum order."""
import os

import numpy as np
import pytest
import torch

import kmeans_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def as_np(t):
    return t.detach().cpu().numpy()


def strided(X, pad, dev):
    """X [n, d] on the device as a view of a [n, d + pad] buffer whose pad columns hold NaN: never read as data"""
    X = torch.as_tensor(X, dtype=torch.float32)
    buf = torch.full((X.shape[0], X.shape[1] + pad), float("nan"), dtype=torch.float32)
    buf[:, :X.shape[1]] = X
    return buf.to(dev)[:, :X.shape[1]]


def raw_step(X, C, labels, status, tol_abs):
    """one gae_kmeans_step on device tensors (X may be a strided view), on a workspace of its own"""
    from gae_dgl_amd import _lib
    from gae_dgl_amd.ops import _ptr, _stream
    n, d = X.shape
    k = C.shape[0]
    nbytes = _lib.load().gae_kmeans_workspace_bytes(n, d, k)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=X.device)
    _lib.call("gae_kmeans_step", _ptr(X), X.stride(0) if n > 1 else d, n, d, _ptr(C), k, _ptr(labels), _ptr(status),
              float(tol_abs), 0, _ptr(ws), ws.numel(), _stream())
    torch.cuda.synchronize()
    st = status.cpu()
    return {"done": int(st[0]), "iterations": int(st[1]), "changed": int(st[2]), "empty": int(st[3]),
            "inertia": float(st[4:5].view(torch.float64)), "shift2": float(st[5:6].view(torch.float64))}


# ------------------------------------------------------------------ assignment
def test_exact_assignment_every_shape(dev):
    """X and C multiples of 1/8 in [-4, 4]: every product, every h_c and every distance is exact in fp32, so labels
    (ties and duplicate centres to the lower index) and dist2 must equal the fp64 reference bit for bit"""
    from gae_dgl_amd import ops
    rng = np.random.default_rng(0)
    cases = 0
    for n in (1, 31, 33, 174, 1025):
        for d in (1, 7, 16, 17, 48, 64):
            for k in (1, 2, 31, 32, 33, 256):
                if k > n:
                    continue
                X = rng.integers(-32, 33, (n, d)) / 8.0
                C = rng.integers(-32, 33, (k, d)) / 8.0
                if k >= 2:
                    C[1] = C[0]
                    C[1, 0] = C[0, 0] + (0.25 if C[0, 0] <= 0 else -0.25)
                    X[0] = C[0]
                    X[0, 0] = (C[0, 0] + C[1, 0]) / 2                  # equidistant from centres 0 and 1
                    C[k - 1] = C[k // 2]                               # duplicate centres (k = 2: of itself)
                    X[n - 1] = C[k - 1]                                # a row ON the duplicated centre
                labels, d2 = ops.kmeans_assign(strided(X, 3, dev), torch.as_tensor(C, dtype=torch.float32).to(dev))
                ref_l, ref_d, _ = R.assign(X, C)
                assert labels.dtype == torch.int32 and d2.dtype == torch.float32
                assert np.array_equal(as_np(labels).astype(np.int64), ref_l), (n, d, k)
                assert np.array_equal(as_np(d2).astype(np.float64), ref_d), (n, d, k)
                cases += 1
    assert cases > 100


@pytest.mark.parametrize("scale", [1.0, 100.0])
@pytest.mark.parametrize("d,k", [(16, 33), (48, 7)])
def test_tolerant_assignment_no_row_exempt(dev, scale, d, k):
    from gae_dgl_amd import ops
    rng = np.random.default_rng(3)
    n = 4099
    X = (scale * rng.standard_normal((n, d))).astype(np.float32)
    C = (X[rng.choice(n, k, replace=False)] + 0.1 * scale * rng.standard_normal((k, d))).astype(np.float32)
    labels, d2 = ops.kmeans_assign(torch.from_numpy(X).to(dev), torch.from_numpy(C).to(dev))
    lab = as_np(labels)
    assert lab.min() >= 0 and lab.max() < k
    excess, allow = R.tolerant_excess(X, C, lab)
    print(f"scale {scale} d {d} k {k}: max excess / allowance {float((excess / allow).max()):.3e}")
    assert (excess <= allow).all()
    own = R.dist2(X, C)[np.arange(n), lab]
    assert np.allclose(as_np(d2), own, rtol=1e-5, atol=0)              # direct: relative accuracy even at scale 100


# ------------------------------------------------------------------ update
@pytest.fixture(scope="module")
def big3():
    return R.blobs(40000, 16, 3, seed=2, noise=1.0)


@pytest.mark.parametrize("n", [1025, 40000])                           # 17 and 507 block partials: both orders
def test_update_matches_segment_means(dev, big3, n):
    X = big3[:n]
    k, d = 3, 16
    C0 = X[:k].copy()
    Xd = torch.from_numpy(X).to(dev)
    C = torch.from_numpy(C0).to(dev)
    labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(6, dtype=torch.int64, device=dev)
    st = raw_step(Xd, C, labels, status, -1.0)
    lab = as_np(labels).astype(np.int64)
    excess, allow = R.tolerant_excess(X, C0, lab)
    assert (excess <= allow).all()
    new, counts, n_empty, shift2 = R.update(X, lab, C0)
    scale = float(np.abs(X).max())
    assert st["iterations"] == 1 and st["changed"] == n and st["empty"] == n_empty == 0 and st["done"] == 0
    assert np.abs(as_np(C).astype(np.float64) - new).max() <= 1e-6 * scale
    inertia = R.dist2(X, C0)[np.arange(n), lab].sum()
    assert abs(st["inertia"] - inertia) <= 1e-6 * inertia
    assert abs(st["shift2"] - shift2) <= 1e-6 * shift2
    # a second step from the same labels: changed counts only the rows that moved
    st2 = raw_step(Xd, C, labels, status, -1.0)
    lab2 = as_np(labels).astype(np.int64)
    assert st2["iterations"] == 2 and st2["changed"] == int((lab2 != lab).sum())


def test_counts_and_empty_cluster(dev, big3):
    from gae_dgl_amd import ops
    X = big3[:4099]
    C0 = np.concatenate([X[:3], np.full((1, 16), 1e3, np.float32)])   # a centre no row is near
    res = ops.kmeans(torch.from_numpy(X).to(dev), 4, init=torch.from_numpy(C0).to(dev), max_iter=1, tol=0)
    lab = as_np(res.labels).astype(np.int64)
    assert res.n_iter == 1 and not res.converged and res.n_empty == 1
    assert np.array_equal(as_np(res.counts), np.bincount(lab, minlength=4)) and res.counts.dtype == torch.int64
    assert int(res.counts[3]) == 0
    assert np.array_equal(as_np(res.centers)[3], C0[3])                # kept, bit for bit
    new = R.update(X, lab, C0)[0]
    assert np.abs(as_np(res.centers).astype(np.float64) - new).max() <= 1e-6 * float(np.abs(X).max())


def test_sums_have_the_same_bits_run_to_run_and_for_any_ldx(dev, big3):
    from gae_dgl_amd import ops
    X = big3
    C0 = torch.from_numpy(X[:3].copy()).to(dev)
    runs = [ops.kmeans(x, 3, init=C0, max_iter=2, tol=0)
            for x in (torch.from_numpy(X).to(dev), torch.from_numpy(X).to(dev), strided(X, 5, dev))]
    for r in runs[1:]:
        assert torch.equal(r.centers, runs[0].centers) and torch.equal(r.labels, runs[0].labels)
        assert r.inertia == runs[0].inertia


# ------------------------------------------------------------------ seeding
SEED_CASES = [(33, 16, 3), (200, 16, 8), (257, 48, 5), (1000, 64, 33)]


@pytest.mark.parametrize("n,d,k", SEED_CASES)
def test_seeding_picks_the_reference_rows(dev, n, d, k):
    from gae_dgl_amd import ops
    X = R.blobs(n, d, k, seed=1)
    Xd = strided(X, 1, dev)
    for seed in range(20):
        ref, gaps = R.seed_pp(X, k, seed)
        assert (gaps > 1e-4).all(), (seed, gaps.min())                 # a closer race would be a bad input, not a skip
        C, chosen = ops.kmeans_init_pp(Xd, k, seed=seed)
        got = as_np(chosen).astype(np.int64)
        assert np.array_equal(got, ref), (seed, got, ref)
        assert len(set(got.tolist())) == k
        assert np.array_equal(as_np(C), X[got])                        # the rows, bit for bit


def test_seeding_with_fewer_distinct_rows_than_centres(dev):
    from gae_dgl_amd import ops
    X = np.repeat(np.array([[1.0, 2.0], [3.0, -1.0]], np.float32), 3, axis=0)      # 6 rows, 2 distinct
    C, chosen = ops.kmeans_init_pp(torch.from_numpy(X).to(dev), 4, seed=5)
    ref, _ = R.seed_pp(X, 4, 5)
    got = as_np(chosen).astype(np.int64)
    assert np.array_equal(got, ref) and got[2] == 0 and got[3] == 0    # every key 0: the lowest index
    res = ops.kmeans(torch.from_numpy(X).to(dev), 4, seed=5, tol=0)    # duplicate centres are legal input
    assert res.converged and res.inertia == 0.0 and int(res.counts.sum()) == 6


# ------------------------------------------------------------------ whole runs
@pytest.mark.parametrize("n,d,k", [(33, 16, 3), (200, 16, 8)])
def test_whole_runs_equal_the_reference(dev, n, d, k):
    from gae_dgl_amd import ops
    X = R.blobs(n, d, k, seed=1)
    Xd = torch.from_numpy(X).to(dev)
    tol_abs = 1e-4 * float(X.astype(np.float64).var(0).mean())
    for seed in range(20):
        chosen, _ = R.seed_pp(X, k, seed)
        ref = R.lloyd(X, X[chosen], tol_abs, 100)
        assert ref["gap"] > 1e-3, (seed, ref["gap"])
        res = ops.kmeans(Xd, k, init="k-means++", seed=seed)
        assert np.array_equal(as_np(res.labels).astype(np.int64), ref["labels"]), seed
        assert res.n_iter == ref["n_iter"] and res.converged == ref["converged"], seed
        assert np.abs(as_np(res.centers) - ref["centers"]).max() <= 1e-5 * max(1.0, np.abs(ref["centers"]).max())
        assert abs(res.inertia - ref["inertia"]) <= 1e-5 * ref["inertia"]
        assert np.array_equal(as_np(res.counts), ref["counts"])


def test_whole_run_on_overlapping_data(dev):
    from gae_dgl_amd import ops
    n, d, k = 4099, 2, 7                                               # two features: the blobs overlap heavily
    X = R.blobs(n, d, k, seed=1, noise=1.5)
    Xd = torch.from_numpy(X).to(dev)
    C0 = torch.from_numpy(X[:k].copy()).to(dev)
    runs = {ce: ops.kmeans(Xd, k, init=C0, tol=0, max_iter=300, check_every=ce) for ce in (1, 8, 64)}
    res = runs[8]
    print(f"overlapping blobs: {res.n_iter} iterations, inertia {res.inertia:.6g}")
    assert res.converged and res.n_iter >= 10                          # the reference takes 41: several groups of 8
    for ce in (1, 64):
        assert torch.equal(runs[ce].labels, res.labels) and torch.equal(runs[ce].centers, res.centers)
        assert runs[ce].inertia == res.inertia and runs[ce].n_iter == res.n_iter and runs[ce].converged
    lab, C = as_np(res.labels).astype(np.int64), as_np(res.centers)
    excess, allow = R.tolerant_excess(X, C, lab)
    assert (excess <= allow).all()                                     # optimal for the returned centres
    means = R.update(X, lab, C)[0]
    assert np.abs(C - means).max() <= 1e-6 * float(np.abs(X).max())    # ... which are the means of the returned labels
    first = R.assign(X, X[:k])[1].sum()
    assert res.inertia <= first
    short = ops.kmeans(Xd, k, init=C0, tol=0, max_iter=3)
    assert not short.converged and short.n_iter == 3


def test_no_fallback_and_argument_errors(dev):
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    X = torch.randn(40, 8, device=dev)
    with pytest.raises(GaeHipError):
        ops.kmeans(X[:3], 4)                                           # k > n
    with pytest.raises(GaeHipError):
        ops.kmeans(torch.randn(40, 65, device=dev), 2)
    bad = X.clone(); bad[7, 3] = float("inf")
    with pytest.raises(GaeHipError):
        ops.kmeans(bad, 2)
    with pytest.raises(GaeHipError):
        ops.kmeans(X.double(), 2)


# ------------------------------------------------------------------ model and scripts
def fresh_graph(g, dev):
    import gae_dgl_amd as G
    gr = G.DGLGraph()
    gr.add_nodes(int(g["n"]))
    gr.add_edges(g["src"], g["dst"])
    gr.to(dev)
    gr.ndata['h'] = torch.from_numpy(g["X"]).to(dev)
    return gr


def test_cluster_nodes_is_kmeans_of_the_embedding(dev):
    import gae_dgl_amd as G
    from gae_dgl_amd import ops
    from gae_dgl_amd.vgae import VGAE
    g = load_golden("sym200")
    model = G.GAE(g["X"].shape[1], [int(h) for h in g["hidden"]])
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd/")})
    model = model.to(dev)
    gr = fresh_graph(g, dev)
    feat = gr.ndata['h']
    res = model.cluster_nodes(gr, 4, seed=3)
    assert gr.ndata['h'] is feat
    with torch.no_grad():
        want = ops.kmeans(model.encode(fresh_graph(g, dev)), 4, seed=3)
    assert torch.equal(res.labels, want.labels) and torch.equal(res.centers, want.centers)
    assert res.inertia == want.inertia and res.n_iter == want.n_iter
    torch.manual_seed(0)
    vg = VGAE(g["X"].shape[1], [32, 16]).to(dev)
    with torch.no_grad():
        mu, _ = vg.encode(fresh_graph(g, dev))
    a, b = vg.cluster_nodes(fresh_graph(g, dev), 3, seed=1), ops.kmeans(mu.contiguous(), 3, seed=1)
    assert torch.equal(a.labels, b.labels) and torch.equal(a.centers, b.centers) and a.inertia == b.inertia


def test_cli_cluster(tmp_path, capsys):
    from gae_dgl_amd import metrics
    from gae_dgl_amd import train_transductive as TT
    rng = np.random.default_rng(0)
    n, k = 300, 3
    comm = rng.integers(0, k, n)
    a = rng.integers(0, n, 6000); b = rng.integers(0, n, 6000)
    keep = (comm[a] == comm[b]) & (a != b)
    a, b = a[keep], b[keep]
    feats = np.eye(k, dtype=np.float32)[comm] + 0.1 * rng.standard_normal((n, k)).astype(np.float32)
    classes = comm.copy(); classes[:10] = -1
    os.makedirs(tmp_path / "data", exist_ok=True)
    np.savez(tmp_path / "data" / "cora.npz", src=np.concatenate([a, b]), dst=np.concatenate([b, a]), features=feats, n=n,
             labels=classes)
    out = tmp_path / "clusters.npz"
    TT.main(["--dataset", "cora", "--data_root", str(tmp_path / "data"), "-e", "20", "-s", str(tmp_path), "--seed", "0",
             "--log_every", "1000", "--cluster", "3", "--cluster_seed", "1", "--cluster_out", str(out)])
    text = capsys.readouterr().out
    line = [l for l in text.splitlines() if l.startswith("NMI:")]
    assert len(line) == 1 and any(l.startswith("k-means K = 3: inertia") for l in text.splitlines()), text
    fields = dict(f.split(":") for f in line[0].split(" | "))
    z = np.load(out)
    assert z["labels"].dtype == np.int32 and z["labels"].shape == (n,) and z["centers"].shape == (3, 16)
    cm = metrics.clustering_metrics(z["labels"], classes)
    assert cm["n"] == n - 10
    for key in ("nmi", "ari", "acc"):
        assert float(fields[key.upper()]) == pytest.approx(cm[key], abs=1e-4)


def test_cli_embed_clusters_on_mol8(tmp_path, capsys, monkeypatch):
    import gae_dgl_amd as G
    from gae_dgl_amd import embed as E
    from gae_dgl_amd.dataset import DeviceGraphDataset
    parts = load_golden("mol8_parts"); whole = load_golden("mol8")
    ng = int(parts["n_graphs"])
    gp = np.zeros(ng + 1, np.int64); np.cumsum([int(parts[f"g{i}/n"]) for i in range(ng)], out=gp[1:])
    src = np.concatenate([parts[f"g{i}/src"] + gp[i] for i in range(ng)])
    dst = np.concatenate([parts[f"g{i}/dst"] + gp[i] for i in range(ng)])
    ds = DeviceGraphDataset(gp, src, dst, whole["X"], device=torch.device("cuda:0"))
    ckpt = str(tmp_path / "mol8.pkl")
    monkeypatch.setattr(E, "load_dataset", lambda args, device: ds)    # the golden molecules as the resident set
    torch.save({k[3:]: torch.from_numpy(v) for k, v in whole.items() if k.startswith("sd/")}, ckpt)
    hidden = [str(int(h)) for h in whole["hidden"]]
    E.main(["--checkpoint", ckpt, "--hidden_dims", *hidden, "--in_dim", str(whole["X"].shape[1]), "--synthetic", str(ng),
            "--out", str(tmp_path / "f.npy"), "--clusters", "3", "--clusters_out", str(tmp_path / "c.npz")])
    assert "Clustered 8 molecules into 3" in capsys.readouterr().out
    z = np.load(tmp_path / "c.npz")
    feats = np.load(tmp_path / "f.npy")
    assert z["labels"].shape == (ng,) and z["centers"].shape == (3, feats.shape[1])
    assert set(z["labels"].tolist()) <= {0, 1, 2}
    lab = R.assign(feats, z["centers"])[0]
    excess, allow = R.tolerant_excess(feats, z["centers"], z["labels"])
    assert (excess <= allow).all() and np.bincount(lab, minlength=3).sum() == ng
