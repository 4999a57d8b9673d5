"""K17 (gae_decoder_bce_sampled, GAE.reconstruction_loss(g, samples=m)) on the CPU: the workspace query and every
argument error need no GPU; the numpy restatement of the sampler (tests/sampled_ref.py) has the properties the
estimator rests on; the CLI and the model refuse what cannot run before touching a device."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampled_ref as R  # noqa: E402

GAE_E_NULL, GAE_E_SIZE, GAE_E_WORKSPACE, GAE_E_RANGE = -1, -2, -5, -6


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    return _lib.load()


def test_entry_point_declared_and_bound(lib):
    from gae_dgl_amd import _lib, ops
    assert "gae_decoder_bce_sampled" in _lib.SIGNATURES and hasattr(lib, "gae_decoder_bce_sampled")
    assert callable(ops.decoder_bce_sampled) and callable(ops.sharded_decoder_bce_sampled)


def _call(lib, **kw):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)       # host memory: an argument error returns before anything is touched
    a = dict(Z=p, mask=None, ldz=16, n=100, d=16, row_begin=0, n_local=100, m=8, indptr=p, indices=p, t_indptr=p,
             t_indices=p, pw=10.0, p_drop=0.0, seed=0, offset=0, draws=None, loss=p, dZ=p, lddz=16, part=None, ws=p,
             nbytes=1 << 40)
    a.update(kw)
    nb = ctypes.c_int64(a["nbytes"])
    rc = lib.gae_decoder_bce_sampled(a["Z"], a["mask"], a["ldz"], a["n"], a["d"], a["row_begin"], a["n_local"],
                                     a["m"], a["indptr"], a["indices"], a["t_indptr"], a["t_indices"], a["pw"],
                                     a["p_drop"], a["seed"], a["offset"], a["draws"], a["loss"], a["dZ"], a["lddz"],
                                     a["part"], a["ws"], ctypes.byref(nb), None)
    return rc, nb.value


def test_workspace_query_without_gpu(lib):
    sizes = {}
    for n in (1, 2708, 19717, 1 << 20, 1 << 24):
        rc, nb = _call(lib, n=n, n_local=n, m=1, ws=None, Z=None, loss=None, dZ=None, nbytes=-1)
        assert rc == 0 and nb > 0, (n, rc, nb)
        sizes[n] = nb
    # O(n d + n_local): the 2^24-node graph needs ~1.1 GB at d = 16, never O(n^2)
    for n, nb in sizes.items():
        assert nb <= n * 16 * 4 + 16 * n + (1 << 20), (n, nb)
    # a row block asks for less than the whole graph's rows
    rc, nb = _call(lib, n=1 << 20, row_begin=1 << 19, n_local=1 << 18, ws=None, nbytes=-1)
    assert rc == 0 and nb < sizes[1 << 20]
    # pointers are never dereferenced by the query (fake device addresses)
    fake = ctypes.c_void_p(16)
    rc, nb = _call(lib, Z=fake, indptr=fake, indices=fake, t_indptr=fake, t_indices=fake, ws=None, nbytes=-1)
    assert rc == 0 and nb > 0


@pytest.mark.parametrize("kw,code,text", [
    (dict(n=-1, n_local=0), GAE_E_SIZE, b"positive"),
    (dict(n=0, n_local=0), GAE_E_SIZE, b"positive"),
    (dict(d=0, ldz=16), GAE_E_SIZE, b"positive"),
    (dict(d=-3), GAE_E_SIZE, b"positive"),
    (dict(n_local=-1), GAE_E_SIZE, b"row window"),
    (dict(row_begin=-1, n_local=10), GAE_E_SIZE, b"row window"),
    (dict(row_begin=50, n_local=51), GAE_E_SIZE, b"row window"),
    (dict(row_begin=100, n_local=1), GAE_E_SIZE, b"row window"),
    (dict(m=0), GAE_E_RANGE, b"m = 0"),
    (dict(m=-4), GAE_E_RANGE, b"m = -4"),
    (dict(m=101), GAE_E_RANGE, b"m = 101"),
    (dict(d=65, ldz=65, lddz=65), GAE_E_RANGE, b"d = 65"),
    (dict(n=1 << 31, n_local=1), GAE_E_SIZE, b"int32"),
    (dict(p_drop=1.0, mask=None), GAE_E_RANGE, b"dropout_p"),
    (dict(p_drop=-0.1), GAE_E_RANGE, b"dropout_p"),
    (dict(ldz=15), GAE_E_SIZE, b"leading dimension"),
    (dict(lddz=8), GAE_E_SIZE, b"leading dimension"),
    (dict(t_indptr=None), GAE_E_NULL, b"A^T"),
    (dict(p_drop=0.5, mask=None), GAE_E_NULL, b"mask"),
    (dict(Z=None), GAE_E_NULL, b"NULL"),
    (dict(loss=None), GAE_E_NULL, b"NULL"),
    (dict(indptr=None), GAE_E_NULL, b"NULL"),
    (dict(nbytes=64), GAE_E_WORKSPACE, b"workspace"),
])
def test_argument_errors_without_gpu(lib, kw, code, text):
    rc, _ = _call(lib, **kw)
    assert rc == code, lib.gae_last_error()
    assert text in lib.gae_last_error()


def test_argument_errors_also_in_the_size_query(lib):
    for kw in (dict(m=0), dict(m=101), dict(d=65, ldz=65, lddz=65), dict(n_local=101), dict(t_indptr=None)):
        rc, _ = _call(lib, ws=None, nbytes=-1, **kw)
        assert rc < 0, kw


def test_loss_only_needs_no_transposed_csr(lib):
    # not an error: without dZ the CSR of A^T is never read (only the query form runs here)
    rc, nb = _call(lib, t_indptr=None, t_indices=None, dZ=None, ws=None, nbytes=-1)
    assert rc == 0 and nb > 0


# ---------------------------------------------------------------------------------------------------- the sampler
CASES = [(n, m) for n in (1, 2, 3, 1000, 4096, 1 << 16, (1 << 16) + 1, 19717) for m in (1, 7, n)
         if m <= n and (m < n or n <= 4096)]


@pytest.mark.parametrize("n,m", CASES)
def test_sampler_permutations(n, m):
    rows = np.arange(n)
    P = R.partners(1234, 5, n, m, rows)
    assert P.shape == (n, m) and P.min() >= 0 and P.max() < n
    # every pi_s is a permutation of [0, n)
    for s in range(m):
        assert np.array_equal(np.sort(P[:, s]), rows), s
    # the m partners of a row are distinct
    Ps = np.sort(P, axis=1)
    assert (np.diff(Ps, axis=1) != 0).all()
    # the inverse formula: i = sigma^-1((sigma(j) - o_s) mod n) has pi_s(i) = j
    I = R.inverse_partners(1234, 5, n, m, rows)
    for s in range(m):
        assert np.array_equal(P[I[:, s], s], rows), s
    if m == n:       # full cover: every ordered pair exactly once
        assert np.array_equal(Ps, np.broadcast_to(rows, (n, n)))


def test_sampler_bijections_round_trip():
    for n in (1, 2, 5, 1 << 10, 12345, (1 << 20) + 3):
        sig, tau = R.sampler(99, 7, n)
        x = np.arange(min(n, 50000), dtype=np.uint64)
        assert np.array_equal(sig.inv(sig.fwd(x).astype(np.uint64)), x.astype(np.int64))
        assert np.array_equal(tau.fwd(tau.inv(x).astype(np.uint64)), x.astype(np.int64))


def test_sampler_depends_on_seed_and_draw():
    n, m = 4096, 8
    a = R.partners(1, 0, n, m, np.arange(n))
    assert not np.array_equal(a, R.partners(1, 1, n, m, np.arange(n)))
    assert not np.array_equal(a, R.partners(2, 0, n, m, np.arange(n)))
    assert np.array_equal(a, R.partners(1, 0, n, m, np.arange(n)))


def test_sampler_partners_look_uniform():
    # column counts of pi over many draws: each column is hit m times per draw exactly (pi_s are permutations); the
    # partners of ONE row over draws spread over [0, n)
    n, m, draws = 257, 4, 2000
    hits = np.zeros(n)
    for t in range(draws):
        hits[R.partners(3, t, n, m, [17])[0]] += 1
    expect = draws * m / n
    assert abs(hits.mean() - expect) < 1e-9
    chi2 = ((hits - expect) ** 2 / expect).sum()
    assert chi2 < n + 6 * np.sqrt(2 * n), chi2


def test_estimate_at_full_cover_is_the_exact_loss():
    # fp64 restatement: m = N covers every pair once, so the estimate is the reference loss and its gradient
    rng = np.random.default_rng(0)
    n, d = 40, 6
    Z = rng.normal(size=(n, d)) * 0.4
    src = rng.integers(0, n, 90); dst = rng.integers(0, n, 90)
    src = np.concatenate([src, [3, 3, 5]]); dst = np.concatenate([dst, [3, 3, 9]])    # self-loop, duplicates
    pw = (n * n - src.size) / src.size
    csr = R.csr_of(dst, src, n)
    csc = R.csr_of(src, dst, n)
    L, G = R.estimate(Z, csr, csc, pw, 11, 2, n)
    L0, G0 = R.exact_loss(Z, src, dst, pw)
    assert abs(L - L0) < 1e-12 * max(1.0, abs(L0))
    assert np.abs(G - G0).max() < 1e-12
    # row blocks: shares sum to the loss, gradient rows are the whole graph's
    parts = [(0, 13), (13, 1), (14, 26)]
    tot = 0.0
    for r0, nl in parts:
        l, g = R.estimate(Z, R.csr_of(dst, src, nl, r0), R.csr_of(src, dst, nl, r0), pw, 11, 2, n, r0, nl)
        tot += l
        assert np.abs(g - G[r0:r0 + nl]).max() < 1e-12
    assert abs(tot - L) < 1e-12


# ---------------------------------------------------------------------------------------------------- host layers
@pytest.mark.parametrize("extra,text", [(["--loss_samples", "0"], "--loss_samples 0: M must be at least 1"),
                                        (["--loss_samples", "-3"], "--loss_samples -3: M must be at least 1")])
def test_cli_refuses_loss_samples(extra, text, capsys, monkeypatch):
    from gae_dgl_amd import train_transductive as TT
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a device was touched"))
    with pytest.raises(SystemExit) as e:
        TT.main(["--dataset", "cora"] + extra)
    assert e.value.code == 2
    assert text in capsys.readouterr().err


def test_cli_accepts_loss_samples():
    from gae_dgl_amd import train_transductive as TT
    assert TT.parse_args(["--loss_samples", "8", "--eval"]).loss_samples == 8
    assert TT.parse_args(["--loss_samples", "1", "--topk", "5", "--eval"]).loss_samples == 1
    assert TT.parse_args([]).loss_samples is None


def _model_and_graph():
    import gae_dgl_amd as G
    from gae_dgl_amd.gae import GAE
    g = G.DGLGraph(([0, 1, 2], [1, 2, 0]), num_nodes=3)
    return GAE(4, [8, 4]), g


@pytest.mark.parametrize("kw,text", [(dict(criterion="mse"), "criterion 'bce'"),
                                     (dict(scope="graph"), "scope 'batch'"),
                                     (dict(samples=0), "positive"),
                                     (dict(samples=2.5), "positive")])
def test_model_refuses_samples_combinations(kw, text, monkeypatch):
    model, g = _model_and_graph()
    kw.setdefault("samples", 4)
    from gae_dgl_amd import _lib
    monkeypatch.setattr(_lib, "call", lambda *a: pytest.fail("a kernel was launched"))
    with pytest.raises(ValueError, match=text):
        model.reconstruction_loss(g, **kw)


def test_vgae_refuses_bad_samples(monkeypatch):
    from gae_dgl_amd import _lib
    from gae_dgl_amd.vgae import VGAE
    import gae_dgl_amd as G
    monkeypatch.setattr(_lib, "call", lambda *a: pytest.fail("a kernel was launched"))
    with pytest.raises(ValueError, match="positive"):
        VGAE(4, (8, 4)).loss(G.DGLGraph(([0], [1]), num_nodes=2), samples=0)


def test_ops_refuse_cpu_tensors():
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    model, g = _model_and_graph()
    with pytest.raises(GaeHipError):
        ops.decoder_bce_sampled(torch.randn(3, 4), None, g, 2)
