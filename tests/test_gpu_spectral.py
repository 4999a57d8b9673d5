"""K32 on the device (gae_spectral_*, ops.spectral_embedding): the bits of tests/spectral_ref.py for every per-element
chain and for the small solve from the device's own Gram pair, the Gram pair inside its rounding bound and bit for bit
against itself, the whole method against LAPACK, the conventions, the failure paths and the downstream path."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import spectral_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = [c.name for c in R.CASES]
DEGREE = 8


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(s=None):
    return ctypes.c_void_p((torch.cuda.current_stream() if s is None else s).cuda_stream)


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.cpu().numpy()


def make_graph(name):
    from gae_dgl_amd import DGLGraph
    g = R.graph(name)
    return DGLGraph((g.src, g.dst), num_nodes=g.n).to(DEV)


class Device:
    """the C ABI on one case's shapes: every entry point on explicit operands"""

    def __init__(self, name):
        from gae_dgl_amd import _lib
        self.lib = _lib
        self.case, self.g = R.BY_NAME[name], R.graph(name)
        self.n, self.b, self.k = self.g.n, R.width(self.case), self.case.k
        self.sigma = 1.0 if self.case.self_loops else 0.0
        self.indptr, self.indices = dev(self.g.indptr), dev(self.g.indices)
        self.nnz = self.indices.shape[0]
        self.ws = torch.empty(_lib.load().gae_spectral_workspace_bytes(self.n, self.nnz, self.b), dtype=torch.uint8, device=DEV)
        self.status = torch.zeros(8, dtype=torch.int64, device=DEV)
        self.s = torch.empty(self.n, dtype=torch.float64, device=DEV)
        _lib.call("gae_spectral_scale", _ptr(self.indptr), self.n, self.sigma, _ptr(self.s), _stream())

    def spmm(self, Yin, Yprev, coef, indices=None):
        out = torch.full_like(Yin, float("nan"))
        cd = dev(np.asarray(coef, np.float64))
        ind = self.indices if indices is None else indices
        self.lib.call("gae_spectral_spmm", _ptr(self.indptr), _ptr(ind), self.n, self.nnz, _ptr(self.s), self.sigma, _ptr(Yin),
                      _ptr(Yprev), _ptr(out), self.b, _ptr(cd), _ptr(self.status), _stream())
        return out

    def gram(self, V, AV, max_blocks=0, stream=None):
        G, H = (torch.full((self.b, self.b), float("nan"), dtype=torch.float64, device=DEV) for _ in range(2))
        self.lib.call("gae_spectral_gram", _ptr(V), _ptr(AV), self.n, self.b, _ptr(G), _ptr(H), max_blocks, _ptr(self.ws),
                      self.ws.numel(), _stream(stream))
        return G, H

    def solve(self, G, H):
        b = self.b
        T = torch.empty(b, b, dtype=torch.float64, device=DEV)
        values = torch.empty(b, dtype=torch.float64, device=DEV)
        coef = torch.zeros(R.MAX_DEGREE + 1, 3, dtype=torch.float64, device=DEV)
        self.lib.call("gae_spectral_solve", _ptr(G), _ptr(H), b, self.k, DEGREE, _ptr(T), _ptr(values), _ptr(coef),
                      _ptr(self.status), _ptr(self.ws), self.ws.numel(), _stream())
        return T, values, coef

    def rotate(self, V, AV, T, values, tol):
        V, AV = V.clone(), AV.clone()
        res = torch.empty(self.b, dtype=torch.float64, device=DEV)
        self.lib.call("gae_spectral_rotate", _ptr(V), _ptr(AV), self.n, self.b, self.k, _ptr(T), _ptr(values), tol, _ptr(res),
                      _ptr(self.status), _ptr(self.ws), self.ws.numel(), _stream())
        return V, AV, res

    def finish(self, V, first, k, values, scaling):
        vec = torch.empty(self.n, k, dtype=torch.float64, device=DEV)
        emb = torch.empty(self.n, k, dtype=torch.float32, device=DEV)
        self.lib.call("gae_spectral_finish", _ptr(V), self.n, self.b, first, k, _ptr(values), _ptr(self.s),
                      {"none": 0, "degree": 1, "value": 2}[scaling], _ptr(vec), _ptr(emb), _ptr(self.ws), self.ws.numel(), _stream())
        return vec, emb


@functools.lru_cache(maxsize=None)
def device(name):
    return Device(name)


@functools.lru_cache(maxsize=None)
def operands(name):
    """(V, AV) numpy [n, b] of a case: the restatement's start block and its plain product, computed once"""
    d = device(name)
    V = R.init(d.n, d.b, 0)[0]
    s = R.scale(d.g.indptr, d.sigma)
    return V, R.spmm(d.g.indptr, d.g.indices, s, d.sigma, V, None, (1.0, 0.0, 0.0))


@functools.lru_cache(maxsize=None)
def embedded(name):
    """ops.spectral_embedding on a case at the defaults, computed once"""
    from gae_dgl_amd import ops
    c = R.BY_NAME[name]
    return ops.spectral_embedding(make_graph(name), c.k, self_loops=c.self_loops, oversample=c.oversample)


@pytest.mark.parametrize("name", NAMES)
def test_scale_and_init(name):
    """the scales bit for bit; the start block within 8 ulp of rad (the fp64 log, sin and cos of the device library are
    not correctly rounded: a few ulp each, on values no larger than rad) from exactly restated uniforms"""
    from gae_dgl_amd import _lib
    d = device(name)
    assert np.array_equal(host(d.s), R.scale(d.g.indptr, d.sigma))
    V = torch.empty(d.n, d.b, dtype=torch.float64, device=DEV)
    _lib.call("gae_spectral_init", _ptr(V), d.n, d.b, 0, _stream())
    ref, rad = R.init(d.n, d.b, 0)
    err = np.abs(host(V) - ref)
    print(f"{name}: start block worst |dev - ref| / (ulp rad) = {(err / (2.0 ** -52 * np.maximum(rad, 1e-300))).max():.2f}")
    assert np.all(err <= 8 * 2.0 ** -52 * rad + 1e-300)
    W = torch.empty_like(V)
    _lib.call("gae_spectral_init", _ptr(W), d.n, d.b, 1, _stream())
    assert not torch.equal(V, W)


@pytest.mark.parametrize("name", NAMES)
def test_spmm_bit_for_bit(name):
    """random alpha, beta, gamma, with and without Yprev; indices read through a base that is 4 bytes off a 16-byte
    boundary give the same bits"""
    d = device(name)
    V, AV = operands(name)
    rng = np.random.default_rng(5)
    coef = rng.standard_normal(3)
    s = R.scale(d.g.indptr, d.sigma)
    Vd, Pd = dev(V), dev(AV)
    for prev in (None, AV):
        want = R.spmm(d.g.indptr, d.g.indices, s, d.sigma, V, prev, coef)
        got = host(d.spmm(Vd, None if prev is None else Pd, coef))
        assert np.array_equal(got, want), (name, prev is None, np.abs(got - want).max())
    shifted = torch.empty(d.nnz + 5, dtype=torch.int32, device=DEV)[1:1 + d.nnz]
    assert shifted.data_ptr() % 16 == 4
    shifted.copy_(d.indices)
    assert np.array_equal(host(d.spmm(Vd, Pd, coef, indices=shifted)), want)
    assert np.array_equal(host(d.spmm(Vd, None, (1.0, 0.0, 0.0))), AV)
    assert int(d.status[4]) == 0


@pytest.mark.parametrize("name", NAMES)
def test_gram_bound_and_determinism(name):
    """|G - V^T V| <= gamma_n sum |v| |w| per entry (and H likewise), gamma_n = n 2^-53 / (1 - n 2^-53); symmetric bit for
    bit; the same bits on a second run, on a grid of 3 blocks and on a non-default stream"""
    d = device(name)
    V, AV = operands(name)
    Vd, Ad = dev(V), dev(AV)
    G, H = d.gram(Vd, Ad)
    Gr, Hr = R.gram(V, AV)
    bG, bH = R.gram_bound(V, AV)
    g, h = host(G), host(H)
    iu = np.triu_indices(d.b)
    assert np.all(np.abs(g - V.T @ V)[iu] <= bG[iu]) and np.all(np.abs(h - V.T @ AV)[iu] <= bH[iu])
    assert np.array_equal(g, g.T) and np.array_equal(h, h.T)
    for kw in (dict(), dict(max_blocks=3), dict(max_blocks=1)):
        G2, H2 = d.gram(Vd, Ad, **kw)
        assert torch.equal(G, G2) and torch.equal(H, H2), kw
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        G3, H3 = d.gram(Vd, Ad, stream=side)
    side.synchronize()
    assert torch.equal(G, G3) and torch.equal(H, H3)


@pytest.mark.parametrize("max_blocks", [0, 1])
@pytest.mark.parametrize("n", [1, 256 + 7, 33 * 256 + 5])
@pytest.mark.parametrize("b", [2, 18, 128])
def test_gram_exact_on_integers(b, n, max_blocks):
    """V and AV hold integers in -3..3, so every product and every sum is exact in any order: the upper triangles of G and
    H ARE V^T V and V^T AV (int64), the lower triangles their mirrors -- the kernel's contract, V^T AV itself is not
    symmetric here.  b: one tile, a ragged second tile, all 36 tile pairs; n: one short chunk, a ragged second chunk, 34
    chunks (the 64-lane order of the partials); on the default grid and on one block"""
    from gae_dgl_amd import _lib
    assert _lib.SPECTRAL_CHUNK_ROWS == 256
    rng = np.random.default_rng(1000 * b + n)
    V, AV = rng.integers(-3, 4, (n, b)), rng.integers(-3, 4, (n, b))
    nbytes = _lib.load().gae_spectral_workspace_bytes(n, 0, b)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    G, H = (torch.full((b, b), float("nan"), dtype=torch.float64, device=DEV) for _ in range(2))
    Vd, Ad = dev(V, torch.float64), dev(AV, torch.float64)
    _lib.call("gae_spectral_gram", _ptr(Vd), _ptr(Ad), n, b, _ptr(G), _ptr(H), max_blocks, _ptr(ws), nbytes, _stream())
    iu, il = np.triu_indices(b), np.tril_indices(b, -1)
    for got, want in ((host(G), V.T @ V), (host(H), V.T @ AV)):
        assert np.array_equal(got[iu], want[iu].astype(np.float64)), np.argwhere(np.triu(got != want))[:4]
        assert np.array_equal(got[il], got.T[il])


@pytest.mark.parametrize("name", NAMES)
def test_solve_rotate_finish_bit_for_bit(name):
    """gae_spectral_solve from the device's own G and H gives the restatement's T, Ritz values, coefficients and info;
    gae_spectral_rotate its blocks, residuals and converged count; gae_spectral_finish its vectors and embeddings"""
    d = device(name)
    V, AV = operands(name)
    Vd, Ad = dev(V), dev(AV)
    G, H = d.gram(Vd, Ad)
    T, values, coef = d.solve(G, H)
    ref = R.solve(host(G), host(H), d.k, DEGREE)
    st = d.status.cpu()
    assert int(st[0]) == ref.info == 0
    assert np.array_equal(host(values), ref.values)
    assert np.array_equal(host(T), ref.T)
    assert np.array_equal(host(coef), ref.coef)
    assert st[5:7].view(torch.float64).tolist() == [ref.values[0], ref.values[d.k - 1]]
    tol = float(np.median(R.rotate(V, AV, ref.T, ref.values, 0.0, d.k)[2][:d.k]))     # some columns pass, some do not
    V2, AV2, res = d.rotate(Vd, Ad, T, values, tol)
    rV, rAV, rres, rconv = R.rotate(V, AV, ref.T, ref.values, tol, d.k)
    assert np.array_equal(host(V2), rV) and np.array_equal(host(AV2), rAV)
    assert np.array_equal(host(res), rres)
    st = d.status.cpu()
    assert int(st[1]) == rconv and int(st[3]) == 0
    assert float(st[7:8].view(torch.float64)) == rres[:d.k].max()
    for scaling in ("none", "degree", "value"):
        for first, k in ((0, d.k), (1, d.k - 1)) if d.k > 1 else ((0, 1), (1, 1)):
            vec, emb = d.finish(V2, first, k, values, scaling)
            rvec, remb = R.finish(rV, first, k, ref.values, R.scale(d.g.indptr, d.sigma), scaling)
            assert np.array_equal(host(vec), rvec) and np.array_equal(host(emb), remb), (scaling, first)


def test_solve_reports_a_rank_deficient_block():
    """two equal columns: the Cholesky's pivot fails, info names it, T and the values are NaN"""
    d = device("n257_b18")
    V, AV = (a.copy() for a in operands("n257_b18"))
    V[:, 7] = V[:, 3]
    AV[:, 7] = AV[:, 3]
    G, H = d.gram(dev(V), dev(AV))
    T, values, _ = d.solve(G, H)
    ref = R.solve(host(G), host(H), d.k, DEGREE)
    assert ref.info > 0 and int(d.status[0]) == ref.info
    assert torch.isnan(T).all() and torch.isnan(values).all()
    d.status.zero_()


@pytest.mark.parametrize("name", NAMES)
def test_end_to_end_against_lapack(name):
    """ops.spectral_embedding meets the CPU file's residual, eigenvalue, projector and defect conditions; its outer
    iteration count is within 2 of the restatement's (the Gram sums differ in order)"""
    res = embedded(name)
    ref = R.run_default(name)
    print(f"{name}: device {res.n_iter} iterations / {res.n_spmm} products, restatement {ref.n_iter} / {ref.n_spmm}")
    assert res.converged and res.info == 0
    assert abs(res.n_iter - ref.n_iter) <= 2
    assert res.n_spmm == res.n_iter + DEGREE * (res.n_iter - 1)
    vec, val, rs = host(res.vectors), host(res.values), host(res.residuals)
    assert np.all(rs <= 1e-8)
    defect = R.check_result(name, vec, val, rs)
    assert defect <= 16 * max(R.qr_defect(n) for n in NAMES)
    assert np.array_equal(host(res.embedding), vec.astype(np.float32))
    at = np.argmax(np.abs(vec), axis=0)
    assert (vec[at, np.arange(vec.shape[1])] > 0).all()                  # the sign rule


def test_same_bits_across_runs_and_check_every():
    from gae_dgl_amd import ops
    c = R.BY_NAME["sbm2708"]
    g = make_graph("sbm2708")
    runs = [ops.spectral_embedding(g, c.k, max_iter=4, check_every=ce) for ce in (1, 1, 4)]
    assert all(r.n_iter == 4 and not r.converged for r in runs)
    for r in runs[1:]:
        assert torch.equal(r.vectors, runs[0].vectors) and torch.equal(r.values, runs[0].values)
        assert torch.equal(r.residuals, runs[0].residuals) and torch.equal(r.embedding, runs[0].embedding)
    full = embedded("sbm2708")
    again = ops.spectral_embedding(g, c.k, oversample=c.oversample)
    assert torch.equal(full.vectors, again.vectors) and full.n_iter == again.n_iter


def test_conventions_and_errors():
    from gae_dgl_amd import DGLGraph, ops
    from gae_dgl_amd._lib import GaeHipError
    g = make_graph("planted700")
    base = embedded("planted700")
    s = torch.from_numpy(R.scale(R.graph("planted700").indptr, 0.0)).to(DEV)
    deg = ops.spectral_embedding(g, 8, oversample=8, scaling="degree")
    val = ops.spectral_embedding(g, 8, oversample=8, scaling="value")
    assert torch.equal(deg.vectors, base.vectors) and torch.equal(val.vectors, base.vectors)
    assert torch.equal(deg.embedding, (base.vectors * s[:, None]).float())
    assert torch.equal(val.embedding, (base.vectors * base.values.clamp_min(0.0).sqrt()[None, :]).float())
    drop = ops.spectral_embedding(g, 7, oversample=8, drop_first=True)
    assert torch.equal(drop.values, base.values[1:]) and torch.equal(drop.vectors, base.vectors[:, 1:])
    one = ops.spectral_embedding(g, 8, max_iter=1)
    assert not one.converged and one.n_iter == 1 and one.n_spmm == 1
    assert torch.isfinite(one.vectors).all() and torch.isfinite(one.embedding).all() and torch.isfinite(one.residuals).all()
    with pytest.raises(GaeHipError, match="outside 1..64"):
        ops.spectral_embedding(g, 65)
    with pytest.raises(GaeHipError, match="outside 1..63"):
        ops.spectral_embedding(g, 64, drop_first=True)
    with pytest.raises(GaeHipError, match="exceeds"):
        ops.spectral_embedding(make_graph("cliques_b2"), 8)
    directed = DGLGraph((np.array([0, 1, 2, 3]), np.array([1, 2, 3, 0])), num_nodes=40).to(DEV)
    with pytest.raises(GaeHipError, match="not symmetric"):
        ops.spectral_embedding(directed, 2)


def test_kmeans_on_the_embedding_recovers_the_planted_classes():
    """NMI of ops.kmeans on the degree-scaled spectral embedding of the planted block model is above the NMI the same call
    gives on a Philox-random embedding of the same shape (gae_spectral_init's normals)"""
    from gae_dgl_amd import _lib, metrics, ops
    g, labels = make_graph("planted700"), R.graph("planted700").labels
    sc = ops.spectral_embedding(g, 8, oversample=8, scaling="degree")
    noise = torch.empty(700, 8, dtype=torch.float64, device=DEV)
    _lib.call("gae_spectral_init", _ptr(noise), 700, 8, 0, _stream())
    nmi = [metrics.clustering_metrics(host(ops.kmeans(z.float().contiguous(), R.N_CLASSES, seed=0).labels), labels)["nmi"]
           for z in (sc.embedding, noise)]
    print(f"NMI spectral {nmi[0]:.4f}, random {nmi[1]:.4f}")
    assert nmi[0] > nmi[1]


def test_train_transductive_prints_the_baseline(tmp_path, capsys):
    from gae_dgl_amd import train_transductive as TT
    TT.main(["--dataset", "cora", "-e", "3", "-s", str(tmp_path), "--seed", "0", "--log_every", "100", "--eval",
             "--spectral", "16", "--spectral_out", str(tmp_path / "sc.npz")])
    out = capsys.readouterr().out
    assert "spectral (16) val ROC-AUC: " in out and "spectral (16) test ROC-AUC: " in out
    last = TT.main.last_spectral
    assert last["result"].embedding.shape[1] == 16 and 0.0 <= last["test"]["auc"] <= 1.0
    saved = np.load(tmp_path / "sc.npz")
    assert saved["embedding"].shape == tuple(last["result"].embedding.shape) and saved["values"].shape == (16,)
    for line in out.splitlines():                                         # the model's own lines are printed as before
        assert line.startswith("spectral") or "spectral" not in line
    assert "\ntest ROC-AUC: " in out and "\nval ROC-AUC: " in out


def test_train_transductive_prints_the_baseline_heads(tmp_path, capsys):
    """with --cluster and --classify the k-means and log-reg lines come a second time, prefixed `spectral`"""
    import os
    from gae_dgl_amd import train_transductive as TT
    g = R.graph("planted700")
    feats = np.random.default_rng(3).standard_normal((g.n, 24)).astype(np.float32)
    os.makedirs(tmp_path / "data", exist_ok=True)
    np.savez(tmp_path / "data" / "cora.npz", src=g.src, dst=g.dst, features=feats, n=g.n, labels=g.labels)
    TT.main(["--dataset", "cora", "--data_root", str(tmp_path / "data"), "-e", "3", "-s", str(tmp_path), "--seed", "0",
             "--log_every", "100", "--eval", "--cluster", "7", "--classify", "--spectral", "8", "--spectral_scaling", "degree",
             "--spectral_self_loops"])
    out = capsys.readouterr().out
    for head in ("k-means K = 7: inertia ", "NMI: ", "LogReg (5-fold CV, lambda = "):
        assert "\n" + head in out and "\nspectral " + head in out, head
    last = TT.main.last_spectral
    assert 0.0 <= last["cluster"]["nmi"] <= 1.0 and 0.0 <= last["classify"]["metrics"]["accuracy"] <= 1.0
