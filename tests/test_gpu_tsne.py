"""K29 on the device (gae_tsne_*, ops.tsne / tsne_affinities, GAE.map_nodes, GAE.map_graphs, the two scripts) against
tests/tsne_ref.py.  Every comparison prints its figure before it asserts.  Each bound is 4 x the largest deviation
measured on an MI355X (DESIGN K29 holds the table) and never above its derivable ceiling:

1. affinities: p against the converged fp64 reference in ulp of fp32 (ceiling: 4 ulp -- the bisection runs in fp64, only
   the final rounding and the last bits of beta are left); the perplexity each row reached;
2. repulsion partials per (row, chunk): |dev - ref| / A for the force, A = sum_j |q^2 (y_i - y_j)| over the chunk, and
   |dev - ref| / z for z (ceiling: chunk 2^-24, the sequential-summation bound of a chunk of fp32 adds);
3. the status block after one iteration (Z, KL, |g|^2) and the map after 1 and 5 iterations, on the rows whose reference
   gradient stays clear of 0 (tests/tsne_ref.py: TRAJECTORY_CASES), relative to the largest displacement;
4. bit equality: run to run, strided Y, a side stream, two half chunk launches, check_every;
5. end to end on blobs: purity, the KL curve, the final KL inside the reference's range over five seeds."""
import os

import numpy as np
import pytest
import torch

import tsne_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
CHUNK = 256                                                             # gae_tsne_chunk for every n used here
# 4 x the largest figure the tests printed on an MI355X; the ceilings: 4 ulp for p, CHUNK 2^-24 for the partials
TOL = {
    "p_ulp": 1.0,                 # measured 0.00 on all cases: the floor is the format's -- two fp64 values that differ in
    #                               their last bits may round to neighbouring fp32 values
    "perplexity": 4 * 8.882e-16,  # relative, of the perplexity a row reached
    "force": 4 * 26.68 * U,       # n = 2708, scale 50
    "z": 4 * 18.36 * U,           # n = 2708, scale 50
    "Z": 4 * 1.332e-8,            # relative, n = 2708
    "kl": 4 * 1.332e-8,           # absolute; the log Z term carries it
    "grad2": 4 * 4.860e-8,        # relative, n = 2708
    "y1": 4 * 1.083e-5,           # n = 2708, of the largest displacement (n = 300: 7.4e-7)
    "y5": 4 * 7.299e-6,           # n = 2708 (n = 300: 3.3e-7)
}
assert TOL["p_ulp"] <= 4.0 and TOL["force"] <= CHUNK * U and TOL["z"] <= CHUNK * U


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as ge
    ge.build()
    return torch.device("cuda:0")


def as_np(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = as_np(a), as_np(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------ 1. affinities
def affinity_rows(k, seed=0, n=65):
    """sorted distances; row 3 holds ties (the minimum among them), row 5 is all equal, row 7 ends in padding"""
    rng = np.random.default_rng(seed)
    d2 = np.sort(rng.gamma(2.0, 1.0, (n, k)).astype(np.float32), 1)
    index = rng.integers(0, n, (n, k)).astype(np.int32)
    d2[3] = np.sort(np.round(d2[3] * 2) / 2 + 0.5)
    d2[5] = 1.25
    if k > 1:
        cut = max(1, k // 2)
        index[7, cut:] = -1
        d2[7, cut:] = np.inf
    return index, d2


@pytest.mark.parametrize("k", [1, 5, 64])
@pytest.mark.parametrize("perplexity", [1.5, 5.0, 20.0])
def test_affinities(k, perplexity, dev):
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    index, d2 = affinity_rows(k)
    args = (torch.from_numpy(index).to(dev), torch.from_numpy(d2).to(dev), perplexity)
    if not perplexity < k:
        with pytest.raises(GaeHipError, match="perplexity"):
            ops.tsne_affinities(*args)
        return
    p, perp = ops.tsne_affinities(*args)
    p, perp = as_np(p), as_np(perp)
    want, want_perp = R.affinities(index, d2, perplexity)
    w32 = want.astype(np.float32)
    # in ulp of the reference value, of 2^-100 below that (such a p adds nothing; fp32 subnormals may be flushed)
    ulp = float((np.abs(p.astype(np.float64) - w32) / np.spacing(np.maximum(w32, np.float32(2.0 ** -100)))).max())
    dperp = float(np.abs(perp / want_perp - 1.0).max())
    dsum = float(np.abs(p.astype(np.float64).sum(1) - 1.0).max())
    print(f"affinities k = {k} perplexity = {perplexity}: p {ulp:.2f} ulp | perplexity rel {dperp:.3e} | sum p - 1 {dsum:.3e}")
    assert p.dtype == np.float32 and perp.dtype == np.float64
    assert ulp <= TOL["p_ulp"] and dperp <= TOL["perplexity"]
    assert dsum <= (k + 1) * U                                          # k roundings of 2^-25 relative, summed
    assert (p[7, max(1, k // 2):] == 0).all()                           # padding
    assert np.allclose(p[5], 1.0 / k, rtol=2 * U)                       # all equal: uniform, perplexity k
    plain = np.ones(65, bool)
    plain[[3, 5, 7]] = False
    assert np.abs(perp[plain] / perplexity - 1.0).max() <= TOL["perplexity"]


def test_affinities_rows_with_fewer_than_two_neighbours(dev):
    from gae_dgl_amd import ops
    index = torch.tensor([[4, -1, -1], [-1, -1, -1], [1, 2, 3]], dtype=torch.int32, device=dev)
    d2 = torch.tensor([[2.0, np.inf, np.inf], [np.inf] * 3, [1.0, 2.0, np.nan]], device=dev)
    p, perp = ops.tsne_affinities(index, d2, 1.5)
    assert as_np(p)[:2].tolist() == [[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]] and as_np(perp)[:2].tolist() == [1.0, 0.0]
    assert as_np(p)[2, 2] == 0.0 and abs(float(perp[2]) - 1.5) < 1e-9   # a non-finite distance is no neighbour


# ------------------------------------------------------------------ 2. repulsion partials
def make_state(Y, dev, P=None, pad=None):
    """TSNEState on Y (numpy); ``pad``: Y as a strided view of a wider buffer whose other columns hold NaN"""
    from gae_dgl_amd import ops
    n = Y.shape[0]
    if pad:
        buf = torch.full((n, 2 + pad), float("nan"), device=dev)
        Yd = buf[:, 1:3]
        Yd.copy_(torch.from_numpy(Y))
    else:
        Yd = torch.from_numpy(Y.copy()).to(dev)
    if P is None:
        csr = (torch.zeros(n + 1, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
               torch.zeros(0, device=dev))
    else:
        csr = tuple(torch.from_numpy(a).to(dev) for a in R.csr_of(P))
    return ops.TSNEState(Yd, *csr)


def partial_errors(Y, part):
    want, A = R.repulsion_partials(Y, CHUNK)
    part = part.astype(np.float64)
    ef = float((np.abs(part[:, :2] - want[:, :2]) / np.maximum(A, 1e-300)[:, None, :]).max())
    ez = float((np.abs(part[:, 2] - want[:, 2]) / np.maximum(want[:, 2], 1e-300)).max())
    return ef, ez


@pytest.mark.parametrize("scale", [1e-4, 1.0, 50.0])
@pytest.mark.parametrize("n", [2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 2708])
def test_repulsion_partials(n, scale, dev):
    from gae_dgl_amd import ops
    assert ops.tsne_chunk(n) == CHUNK
    Y = (scale * np.random.default_rng(n).standard_normal((n, 2))).astype(np.float32)
    st = make_state(Y, dev)
    st.partials().fill_(float("nan"))
    st.repulsion(gated=False)
    part = as_np(st.partials())
    assert part.shape == (-(-n // CHUNK), 3, n)
    ef, ez = partial_errors(Y, part)
    print(f"repulsion n = {n} scale = {scale:g}: force {ef / U:.2f} u | z {ez / U:.2f} u  (u = 2^-24)")
    assert ef <= TOL["force"] and ez <= TOL["z"]
    if n % CHUNK == 1 and n > 1:
        assert part[-1, :, n - 1].tolist() == [0.0, 0.0, 0.0]           # the last chunk holds only the row itself


def test_repulsion_duplicated_rows_and_strided_input(dev):
    Y = np.repeat(np.float32([[0.37, -1.2]]), 65, 0)
    st = make_state(Y, dev)
    st.repulsion(gated=False)
    part = as_np(st.partials())
    assert (part[0, :2] == 0).all() and (part[0, 2] == 64.0).all()      # q = rcp(1) = 1 per twin, force exactly 0
    rng = np.random.default_rng(4)
    Y = rng.standard_normal((513, 2)).astype(np.float32)
    Y[100], Y[400] = Y[7], Y[7]
    a, b = make_state(Y, dev), make_state(Y, dev, pad=3)
    assert b.ldy == 5 and b.Y.data_ptr() % 8 == 4                        # rows 20 bytes apart, 4 bytes off an 8-byte line
    a.repulsion(gated=False)
    b.repulsion(gated=False)
    assert same_bits(a.partials(), b.partials()) and np.isfinite(as_np(a.partials())).all()
    ef, ez = partial_errors(Y, as_np(a.partials()))
    assert ef <= TOL["force"] and ez <= TOL["z"]


# ------------------------------------------------------------------ 3. iterations against the reference
def schedule(it, exaggeration_iters=2):
    return (12.0, 0.5) if it < exaggeration_iters else (1.0, 0.8)


@pytest.mark.parametrize("n", [300, 2708])
def test_iterations_follow_the_reference(n, dev):
    _, _, P, Y0 = R.case(n, **R.TRAJECTORY_CASES[n])
    ys, keep = R.trajectory(n)
    assert (~keep).sum() <= 0.02 * n
    st = make_state(Y0, dev, P)
    ref0 = R.gradient(Y0, P, 12.0)
    errs = {}
    for it in range(5):
        st.step(*schedule(it), R.TRAJECTORY_ETA)
        if it == 0:
            s = st.read()
            vals = P[P > 0]
            kl = float((vals * np.log(vals)).sum()) + float(vals.sum()) * s["log_z"] + s["p_log_d"]
            errs["Z"] = abs(s["z"] / ref0["Z"] - 1.0)
            errs["kl"] = abs(kl - R.kl(Y0, P))
            errs["grad2"] = abs(s["grad2"] / float((ref0["g"] ** 2).sum()) - 1.0)
            assert s["iteration"] == 1 and s["nonfinite"] == 0 and s["done"] == 0
        if it in (0, 4):
            move = np.abs(ys[it] - Y0).max()
            errs["y1" if it == 0 else "y5"] = float(np.abs(as_np(st.Y).astype(np.float64) - ys[it])[keep].max() / move)
    print(f"iterations n = {n}: " + " | ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert st.read()["iteration"] == 5
    for k, v in errs.items():
        assert v <= TOL[k], k


# ------------------------------------------------------------------ 4. bit equality
def run_iterations(st, iters=12, halves=False):
    for it in range(iters):
        if halves:
            half = st.chunks // 2
            st.repulsion(half, st.chunks)
            st.repulsion(0, half)
        else:
            st.repulsion()
        st.update(*schedule(it), 50.0)
    return st


def test_same_bits_run_to_run_strided_streamed_and_in_halves(dev):
    _, _, P, Y0 = R.case(300, **R.TRAJECTORY_CASES[300])
    a = run_iterations(make_state(Y0, dev, P))
    assert not same_bits(a.Y, torch.from_numpy(Y0)) and np.isfinite(as_np(a.Y)).all()
    b = run_iterations(make_state(Y0, dev, P))
    c = run_iterations(make_state(Y0, dev, P, pad=3))
    d = run_iterations(make_state(Y0, dev, P), halves=True)
    side = torch.cuda.Stream(device=dev)
    e = make_state(Y0, dev, P)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        run_iterations(e)
    side.synchronize()
    assert a.chunks == 2
    for other in (b, c, d, e):
        assert same_bits(a.Y, other.Y.contiguous()) and same_bits(a.gains, other.gains) and same_bits(a.velocity, other.velocity)
        assert torch.equal(a.status, other.status)
    assert np.isnan(as_np(c.Y._base if c.Y._base is not None else c.Y)[:, 0]).all()      # the pad columns were left alone


def test_same_bits_for_any_check_every(dev):
    from gae_dgl_amd import ops
    X = torch.from_numpy(R.case(300, **R.TRAJECTORY_CASES[300])[0]).to(dev)
    kw = dict(perplexity=5.0, n_iter=20, exaggeration_iters=5, seed=3)
    runs = [ops.tsne(X, check_every=c, **kw) for c in (1, 7, 50)]
    assert [len(r.kl_curve) for r in runs] == [20, 3, 1] and all(r.n_iter == 20 for r in runs)
    for r in runs[1:]:
        assert same_bits(runs[0].embedding, r.embedding) and r.kl_divergence == runs[0].kl_divergence
    assert runs[0].kl_curve[6] == runs[1].kl_curve[0] and runs[0].kl_curve[-1] == runs[2].kl_curve[0]
    wide = torch.full((300, 20), float("nan"), device=dev)
    wide[:, :16] = X
    assert same_bits(ops.tsne(wide[:, :16], check_every=50, **kw).embedding, runs[0].embedding)      # a row stride of X
    assert same_bits(ops.tsne_init(300, 3, dev), torch.from_numpy(R.init(300, 3)))                  # the start, bit for bit
    nb = ops.knn(X, k=15)
    assert same_bits(ops.tsne(X, neighbours=nb, init=ops.tsne_init(300, 3, dev), check_every=50, **kw).embedding,
                     runs[0].embedding)


# ------------------------------------------------------------------ 5. end to end
def test_blobs_end_to_end(dev):
    from gae_dgl_amd import ops
    X, classes, P = R.end_to_end_inputs()
    e = R.END_TO_END
    res = ops.tsne(torch.from_numpy(X).to(dev), perplexity=e["perplexity"], n_iter=e["n_iter"], seed=0, check_every=10)
    Y = as_np(res.embedding)
    assert Y.shape == (e["n"], 2) and Y.dtype == np.float32 and np.isfinite(Y).all() and res.n_iter == e["n_iter"]
    assert np.abs(as_np(res.perplexities) / e["perplexity"] - 1.0).max() <= TOL["perplexity"]
    late = [kl for it, kl in res.kl_curve if it >= 260]
    purity = R.label_purity(Y, classes)
    kl = R.kl(Y, P)
    lo, hi, sd = min(R.END_TO_END_KL), max(R.END_TO_END_KL), float(np.std(R.END_TO_END_KL))
    print(f"blobs: purity {purity} | final KL {kl:.6f} (reference seeds: {lo:.6f} .. {hi:.6f}, sd {sd:.6f}) | "
          f"reported KL {res.kl_divergence:.6f} | |g| {res.grad_norm:.3e} | late curve {np.round(late, 4).tolist()}")
    assert len(late) == 5 and all(a > b for a, b in zip(late, late[1:]))
    assert purity == 1.0
    assert lo - sd <= kl <= hi + sd
    assert abs(res.kl_divergence - kl) < 0.05 and res.kl_divergence == res.kl_curve[-1][1]      # one update apart


def fresh_graph(g, dev):
    import gae_dgl_amd as G
    gr = G.DGLGraph()
    gr.add_nodes(int(g["n"]))
    gr.add_edges(g["src"], g["dst"])
    gr.to(dev)
    gr.ndata['h'] = torch.from_numpy(g["X"]).to(dev)
    return gr


@pytest.mark.parametrize("name,kw", [("tiny", dict(perplexity=2.0, n_iter=20)), ("mol8", dict(n_iter=20))])
def test_map_nodes_of_gae_and_vgae(name, kw, dev):
    import gae_dgl_amd as G
    from gae_dgl_amd import ops
    from gae_dgl_amd.vgae import VGAE
    g = load_golden(name)
    model = G.GAE(g["X"].shape[1], [int(h) for h in g["hidden"]])
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd/")})
    model = model.to(dev)
    gr = fresh_graph(g, dev)
    feat = gr.ndata['h']
    res = model.map_nodes(gr, **kw)
    assert gr.ndata['h'] is feat and res.embedding.shape == (int(g["n"]), 2) and bool(torch.isfinite(res.embedding).all())
    with torch.no_grad():
        assert same_bits(res.embedding, ops.tsne(model.encode(fresh_graph(g, dev)), **kw).embedding)
    torch.manual_seed(0)
    vg = VGAE(g["X"].shape[1], [8, 4]).to(dev)
    gr = fresh_graph(g, dev)
    feat = gr.ndata['h']
    res = vg.map_nodes(gr, **kw)
    assert gr.ndata['h'] is feat and res.embedding.shape == (int(g["n"]), 2) and bool(torch.isfinite(res.embedding).all())
    with torch.no_grad():
        mu = vg.encode(fresh_graph(g, dev))[0]
    assert same_bits(res.embedding, ops.tsne(mu, **kw).embedding)


def test_map_graphs_is_tsne_of_the_molecule_features(dev):
    import gae_dgl_amd as G
    from gae_dgl_amd import ops
    from gae_dgl_amd.dataset import DeviceGraphDataset
    parts, whole = load_golden("mol8_parts"), load_golden("mol8")
    ng = int(parts["n_graphs"])
    gp = np.zeros(ng + 1, np.int64)
    np.cumsum([int(parts[f"g{i}/n"]) for i in range(ng)], out=gp[1:])
    ds = DeviceGraphDataset(gp, np.concatenate([parts[f"g{i}/src"] + gp[i] for i in range(ng)]),
                            np.concatenate([parts[f"g{i}/dst"] + gp[i] for i in range(ng)]),
                            np.concatenate([parts[f"g{i}/X"] for i in range(ng)]), device=dev)
    model = G.GAE(39, [int(h) for h in whole["hidden"]])
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in whole.items() if k.startswith("sd/")})
    model = model.to(dev).eval()
    kw = dict(perplexity=3.0, n_iter=20, seed=1)
    res = model.map_graphs(ds, fused="auto", **kw)
    assert res.embedding.shape == (ng, 2) and bool(torch.isfinite(res.embedding).all()) and res.n_iter == 20
    assert same_bits(res.embedding, ops.tsne(model.embed_graphs(ds), **kw).embedding)
    with pytest.raises(ValueError):
        model.map_graphs(ds, grad=True)


def test_cli_embed_map(tmp_path, capsys):
    from gae_dgl_amd import embed as E
    import gae_dgl_amd as G
    torch.manual_seed(0)
    ckpt = str(tmp_path / "m.pkl")
    torch.save(G.GAE(39, [32, 16]).state_dict(), ckpt)
    E.main(["--checkpoint", ckpt, "--hidden_dims", "32", "16", "--synthetic", "300", "--out", str(tmp_path / "f.npy"),
            "--map_out", str(tmp_path / "map.npz"), "--map_iters", "30", "--map_seed", "2", "--neighbours", "5"])
    text = capsys.readouterr().out
    line = [l for l in text.splitlines() if l.startswith("t-SNE (perplexity 20, 30 iterations) KL: ")]
    assert len(line) == 1 and " | 10-NN preservation: " in line[0] and "Searched 300 molecules" in text, text
    z = np.load(tmp_path / "map.npz")
    assert sorted(z.files) == ["embedding", "kl_curve", "kl_divergence", "labels"]
    assert z["embedding"].shape == (300, 2) and z["embedding"].dtype == np.float32 and (z["labels"] == -1).all()
    assert np.array_equal(z["embedding"], as_np(E.main.map.embedding)) and z["kl_curve"].shape == (1, 2)
    assert f"KL: {float(z['kl_divergence']):.4f} | 10-NN preservation: {E.main.map_preservation:.4f}" in line[0]
    assert 0.0 <= E.main.map_preservation <= 1.0


def test_cli_train_transductive_map(tmp_path, capsys):
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
    out = tmp_path / "map.npz"
    TT.main(["--dataset", "cora", "--data_root", str(tmp_path / "data"), "-e", "10", "-s", str(tmp_path), "--seed", "0",
             "--log_every", "1000", "--map_out", str(out), "--map_perplexity", "10", "--map_iters", "40"])
    text = capsys.readouterr().out
    line = [l for l in text.splitlines() if l.startswith("t-SNE (perplexity 10, 40 iterations) KL: ")]
    assert len(line) == 1 and " | 10-NN preservation: " in line[0], text
    z = np.load(out)
    assert z["embedding"].shape == (n, 2) and np.array_equal(z["labels"], comm) and np.isfinite(z["embedding"]).all()
    assert np.array_equal(z["embedding"], as_np(TT.main.last_map["result"].embedding))
    with pytest.raises(SystemExit):
        TT.parse_args(["--dataset", "cora", "--map_iters", "5"])


def test_errors_and_edges(dev):
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    X = torch.from_numpy(R.case(300, **R.TRAJECTORY_CASES[300])[0]).to(dev).clone()
    bad = X.clone()
    bad[17, 3] = float("nan")
    with pytest.raises(GaeHipError, match="non-finite"):
        ops.tsne(bad, n_iter=5)
    far = torch.full((300, 2), 3e38, device=dev)
    far[::2] = -3e38                                                    # y_i - y_j overflows: 0 x inf in the first sweep
    with pytest.raises(GaeHipError, match="left the finite range"):
        ops.tsne(X, perplexity=5.0, n_iter=10, init=far, check_every=5)
    with pytest.raises(GaeHipError):
        ops.tsne(X, perplexity=5.0, init=torch.zeros(299, 2, device=dev))
    with pytest.raises(GaeHipError):
        ops.tsne(X[:2], perplexity=1.0)                                 # k = 1 admits no perplexity
    with pytest.raises(GaeHipError):
        ops.tsne(torch.zeros(10, 300, device=dev))                      # d beyond ops.knn's 256
    empty = ops.tsne(X[:0])
    assert empty.embedding.shape == (0, 2) and empty.n_iter == 0 and empty.kl_curve == []
    one = ops.tsne(X[:1], seed=4)
    assert same_bits(one.embedding, torch.from_numpy(R.init(1, 4))) and one.n_iter == 0
    given = torch.tensor([[0.5, -0.25]], device=dev)
    assert same_bits(ops.tsne(X[:1], init=given).embedding, given)
    # an early stop on the device: min_grad_norm above every gradient stops after the first update, for any grouping
    r1 = ops.tsne(X, perplexity=5.0, n_iter=20, min_grad_norm=1e3, check_every=1)
    r7 = ops.tsne(X, perplexity=5.0, n_iter=20, min_grad_norm=1e3, check_every=7)
    assert r1.n_iter == 1 == r7.n_iter and same_bits(r1.embedding, r7.embedding)
