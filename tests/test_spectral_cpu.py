"""K32 without a GPU: the numpy restatement tests/spectral_ref.py (what the device must reproduce) against LAPACK on the
dense operator, its iteration counts, the pieces it rests on (the fp64 fma, the packing that lets K31's solver run as it
stands) and the argument errors of every entry point through the C ABI."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import pca_ref
import spectral_ref as R

GAE_E_NULL, GAE_E_SIZE, GAE_E_WORKSPACE, GAE_E_RANGE = -1, -2, -5, -6
NAMES = [c.name for c in R.CASES]
MAX_ITER = 200


def test_fma64_rounds_once():
    """the emulation equals the correctly rounded a b + c (exact rationals), cancellation included, and differs from the
    two-step form"""
    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(2000) for _ in range(3))
    c[::2] = -(a * b)[::2] + c[::2] * 1e-17                             # the sum cancels to the product's rounding error
    got = R.fma64(a, b, c)
    for i in range(2000):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        assert float(exact) == got[i], i                                # float(Fraction) rounds to nearest even
    assert (got != a * b + c).any()
    assert R.fma64(0.0, 5.0, -0.0) == 0.0 and R.fma64(2.0, 3.0, 1.0) == 7.0


def test_packing_returns_the_matrix_bit_for_bit():
    """K31's centring of the packed triangle (S[0][0] = 2, S[0][1..] = 0, S_xx = H') is (H' - 0 . 0) / 1 = H' exactly, so
    gae_pca_solve diagonalises H' as it stands"""
    rng = np.random.default_rng(1)
    for b in (2, 16, 18, 128):
        M = rng.standard_normal((b, b)) * 10.0 ** rng.integers(-8, 8, (b, b))
        Hp = np.triu(M) + np.triu(M, 1).T
        c, mean, C = pca_ref.centre(R.pack(Hp), b, 0, None)
        assert c == 2.0 and not mean.any()
        assert np.array_equal(C, Hp)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_against_lapack(name):
    """Every case converges at tol = 1e-8 within the cap of 200 outer iterations (degree 8), and the converged result meets
    spectral_ref.check_result: reported residuals = recomputed ones, every value within its residual of LAPACK's value
    of the same rank, the Davis-Kahan projector bound for every eigenvalue cluster inside the top k with the gap taken
    from LAPACK's spectrum.
    Outer iterations / block products of the restatement: cycle64 7 / 55, cliques_b2 12 / 100, cliques_loops 3 / 19,
    star300 3 / 19, n257_b18 10 / 82, n255_b128 5 / 37, n256_loops 10 / 82, multi100 7 / 55, planted700 9 / 73,
    sbm2708 (156 components, 58 isolated nodes, the top 16 values all 1) 17 / 145."""
    r = R.run_default(name)
    print(f"{name}: {r.n_iter} outer iterations, {r.n_spmm} products, residual max {r.residuals.max():.2e}")
    assert r.info == 0 and r.converged and r.n_iter <= MAX_ITER
    assert np.all(r.residuals <= 1e-8)
    R.check_result(name, r.vectors, r.values, r.residuals)


def test_orthogonality_defect_against_qr():
    """||V^T V - I||_F of every case is held at 16 x the worst defect numpy.linalg.qr leaves on a block of the same shape
    (test_pca_cpu.py's margin, for the same reason: a different constant, the same backward stability).  Measured: worst
    5.3e-15 (n255_b128) against qr's worst 4.9e-15; the bound is 7.8e-14."""
    worst = max(R.qr_defect(n) for n in NAMES)
    for name in NAMES:
        r = R.run_default(name)
        d = float(np.linalg.norm(r.vectors.T @ r.vectors - np.eye(r.vectors.shape[1])))
        print(f"{name}: defect {d:.3e} (qr {R.qr_defect(name):.3e})")
        assert d <= 16 * worst, (name, d, worst)


def test_known_spectra():
    """the cycle's values are cos(2 pi j / n), each doubly repeated; the disjoint cliques give the repeated value 1"""
    r = R.run_default("cycle64")
    want = np.cos(2 * np.pi * np.array([0, 1, 1, 2, 2]) / 64)
    assert np.all(np.abs(r.values - want) <= 1e-14)
    r = R.run_default("cliques_loops")
    assert np.all(np.abs(r.values - 1.0) <= 1e-14)
    g = R.graph("cliques_b2")
    assert (R.scale(g.indptr, 0.0)[12:] == 0.0).all()                   # isolated nodes: s_i = 0


def test_floor_is_what_lets_the_repeated_one_converge():
    """Without the floor theta_k - 0.02 the interval closes on a block inside the eigenspace of the repeated eigenvalue 1:
    the same case does not reach 1e-8 in the iterations the floored filter needs"""
    with_floor = R.run_default("cliques_b2")
    old = R.FLOOR
    try:
        R.FLOOR = 0.0
        without = R.run("cliques_b2", max_iter=with_floor.n_iter)
    finally:
        R.FLOOR = old
    assert with_floor.converged and not without.converged


def test_conventions():
    r = R.run_default("planted700")
    X = r.vectors
    at = np.argmax(np.abs(X), axis=0)
    assert (X[at, np.arange(X.shape[1])] > 0).all()
    _, zd = R.finish(r.V, 0, 8, r.values, r.s, "degree")
    _, zv = R.finish(r.V, 0, 8, r.values, r.s, "value")
    assert np.array_equal(zd, (X * r.s[:, None]).astype(np.float32))
    assert np.array_equal(zv, (X * np.sqrt(np.maximum(r.values, 0.0))[None, :]).astype(np.float32))
    X1, _ = R.finish(r.V, 1, 7, r.values, r.s, "none")
    assert np.array_equal(X1, X[:, 1:])


def test_sum_partials_orders():
    rng = np.random.default_rng(2)
    p = rng.standard_normal((100, 3))
    lanes = [sum((p[q] for q in range(l, 100, 64)), np.zeros(3)) for l in range(64)]
    for off in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[l] + lanes[l + off] if l + off < len(lanes) else lanes[l] for l in range(len(lanes))]
    assert np.array_equal(R.sum_partials(p), lanes[0])
    seq = np.zeros(3)
    for q in range(32):
        seq = seq + p[q]
    assert np.array_equal(R.sum_partials(p[:32]), seq)


# ------------------------------------------------------------------------------------------------ the C ABI, no GPU
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def p():
    buf = ctypes.create_string_buffer(64)
    return ctypes.cast(buf, ctypes.c_void_p), buf


def test_workspace_is_a_pure_host_function(lib):
    f = lib.gae_spectral_workspace_bytes
    sizes = [f(1000, 5000, b) for b in range(2, 129, 2)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes == [f(1000, 0, b) for b in range(2, 129, 2)]
    assert f(1, 0, 32) < f(257, 0, 32) < f(100000, 0, 32)
    assert f(256, 0, 32) == f(1, 0, 32)                                 # whole chunks of 256 rows
    for b in (0, 1, 3, 130, -2):
        assert f(1000, 0, b) == GAE_E_RANGE
    assert b"even" in lib.gae_last_error()
    for n in (0, -1, 2 ** 31):
        assert f(n, 0, 32) == GAE_E_SIZE
    assert f(10, -1, 32) == GAE_E_SIZE and f(10, 2 ** 31, 32) == GAE_E_SIZE


def test_argument_errors_need_no_gpu(lib, p):
    p = p[0]
    need = lib.gae_spectral_workspace_bytes(100, 400, 16)

    def scale(indptr=p, n=100, sigma=0.0, s=p):
        return lib.gae_spectral_scale(indptr, n, sigma, s, None)
    assert scale(sigma=-1.0) == GAE_E_RANGE and scale(sigma=float("nan")) == GAE_E_RANGE
    assert scale(n=0) == GAE_E_SIZE and scale(n=2 ** 31) == GAE_E_SIZE
    assert scale(indptr=None) == GAE_E_NULL and scale(s=None) == GAE_E_NULL

    def init(V=p, n=100, b=16):
        return lib.gae_spectral_init(V, n, b, 0, None)
    assert init(b=17) == GAE_E_RANGE and init(b=130) == GAE_E_RANGE and init(n=0) == GAE_E_SIZE and init(V=None) == GAE_E_NULL

    def spmm(indptr=p, indices=p, n=100, nnz=400, s=p, sigma=0.0, yin=p, yprev=None, yout=ctypes.c_void_p(p.value + 16), b=16,
             coef=p, status=None):
        return lib.gae_spectral_spmm(indptr, indices, n, nnz, s, sigma, yin, yprev, yout, b, coef, status, None)
    assert spmm(b=0) == GAE_E_RANGE and spmm(b=15) == GAE_E_RANGE and spmm(sigma=-0.5) == GAE_E_RANGE
    assert spmm(n=0) == GAE_E_SIZE and spmm(nnz=-1) == GAE_E_SIZE and spmm(nnz=2 ** 31) == GAE_E_SIZE
    assert spmm(yout=p) == GAE_E_SIZE and b"aliases" in lib.gae_last_error()
    assert spmm(yin=ctypes.c_void_p(p.value + 8)) == GAE_E_SIZE and b"aligned" in lib.gae_last_error()
    for name in ("indptr", "indices", "s", "yin", "yout", "coef"):
        assert spmm(**{name: None}) == GAE_E_NULL, name

    def gram(V=p, AV=p, n=100, b=16, G=p, H=p, max_blocks=0, ws=p, nbytes=need):
        return lib.gae_spectral_gram(V, AV, n, b, G, H, max_blocks, ws, nbytes, None)
    assert gram(b=1) == GAE_E_RANGE and gram(n=0) == GAE_E_SIZE and gram(max_blocks=-1) == GAE_E_SIZE
    for name in ("V", "AV", "G", "H", "ws"):
        assert gram(**{name: None}) == GAE_E_NULL, name
    assert gram(nbytes=need - 1) == GAE_E_WORKSPACE and b"needed" in lib.gae_last_error()

    def solve(G=p, H=p, b=16, k=4, degree=8, T=p, values=p, coef=p, status=p, ws=p, nbytes=need):
        return lib.gae_spectral_solve(G, H, b, k, degree, T, values, coef, status, ws, nbytes, None)
    assert solve(b=130) == GAE_E_RANGE and solve(k=0) == GAE_E_RANGE and solve(k=17) == GAE_E_RANGE
    assert solve(b=128, k=65, nbytes=2 ** 40) == GAE_E_RANGE
    assert solve(degree=0) == GAE_E_RANGE and solve(degree=13) == GAE_E_RANGE
    for name in ("G", "H", "T", "values", "coef", "status", "ws"):
        assert solve(**{name: None}) == GAE_E_NULL, name
    assert solve(nbytes=lib.gae_spectral_workspace_bytes(1, 0, 16) - 1) == GAE_E_WORKSPACE

    def rotate(V=p, AV=ctypes.c_void_p(p.value + 16), n=100, b=16, k=4, T=p, values=p, tol=1e-8, res=p, status=p, ws=p,
               nbytes=need):
        return lib.gae_spectral_rotate(V, AV, n, b, k, T, values, tol, res, status, ws, nbytes, None)
    assert rotate(b=3) == GAE_E_RANGE and rotate(k=17) == GAE_E_RANGE and rotate(tol=-1.0) == GAE_E_RANGE
    assert rotate(tol=float("inf")) == GAE_E_RANGE and rotate(n=0) == GAE_E_SIZE and rotate(AV=p) == GAE_E_SIZE
    for name in ("V", "AV", "T", "values", "res", "status", "ws"):
        assert rotate(**{name: None}) == GAE_E_NULL, name
    assert rotate(nbytes=need - 1) == GAE_E_WORKSPACE

    def finish(V=p, n=100, b=16, first=0, k=4, values=p, s=p, scaling=0, vectors=p, emb=p, ws=p, nbytes=need):
        return lib.gae_spectral_finish(V, n, b, first, k, values, s, scaling, vectors, emb, ws, nbytes, None)
    assert finish(b=18, k=0) == GAE_E_RANGE and finish(scaling=3) == GAE_E_RANGE and finish(scaling=-1) == GAE_E_RANGE
    assert finish(n=2 ** 31) == GAE_E_SIZE and finish(first=13) == GAE_E_SIZE and finish(first=-1) == GAE_E_SIZE
    for name in ("V", "values", "s", "vectors", "emb", "ws"):
        assert finish(**{name: None}) == GAE_E_NULL, name
    assert finish(nbytes=need - 1) == GAE_E_WORKSPACE


def test_python_argument_errors_need_no_gpu(lib):
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    for kw in (dict(k=65), dict(k=0), dict(k=64, drop_first=True), dict(k=16, oversample=1), dict(k=64, oversample=66),
               dict(degree=13), dict(degree=0), dict(scaling="rows"), dict(tol=-1.0), dict(max_iter=0), dict(check_every=0)):
        with pytest.raises(GaeHipError):
            ops.spectral_embedding(None, **kw)
