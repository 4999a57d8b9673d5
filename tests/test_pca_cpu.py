"""K31 without a GPU: the numpy restatement tests/pca_ref.py (what the device must reproduce bit for bit) against the
independent answer -- fp64 covariance and LAPACK's eigh --, its conventions, and the argument errors of the three entry
points through the C ABI."""
import ctypes
import functools

import numpy as np
import pytest

import pca_ref as R

GAE_E_NULL, GAE_E_SIZE, GAE_E_WORKSPACE, GAE_E_RANGE = -1, -2, -5, -6


@functools.lru_cache(maxsize=None)
def solved(name):
    """(X of the listed rows, Solved with all d components) of a case, computed once"""
    case = next(c for c in R.CASES if c[0] == name)
    X, rows, _ = R.make(case)
    Xl = X if rows is None else X[rows]
    d = X.shape[1]
    piv = np.concatenate([Xl.mean(0, dtype=np.float32), Xl[:, :1].mean(0, dtype=np.float32)]).astype(np.float32)
    return Xl, R.solve(R.moments(Xl, piv), d, 1, piv, d)


def figures(C, values, comps):
    """(relative residual |C V - V L|_F / |C|_F, orthogonality defect |V V^T - I|_F); comps holds the vectors as rows"""
    norm = np.linalg.norm(C)
    res = np.linalg.norm(C @ comps.T - comps.T * values[None, :])
    return (res / norm if norm > 0 else res), np.linalg.norm(comps @ comps.T - np.eye(comps.shape[0]))


@functools.lru_cache(maxsize=None)
def table():
    """name -> (residual, defect, LAPACK's residual, LAPACK's defect, |C|_F, largest eigenvalue difference)"""
    out = {}
    for case in R.CASES:
        _, s = solved(case[0])
        w, V = np.linalg.eigh(s.cov)
        w, Vr = w[::-1], V[:, ::-1].T
        r, o = figures(s.cov, s.all_values, s.all_components)
        rl, ol = figures(s.cov, w, Vr)
        out[case[0]] = (r, o, rl, ol, np.linalg.norm(s.cov), np.abs(s.all_values - w).max())
    return out


def test_restatement_is_as_accurate_as_lapack():
    """Both methods are backward stable; the restatement's residual and orthogonality defect are held at 16 x LAPACK's
    worst figure over the case list (the margin covers the different constant: ~13 sweeps of d - 1 rotations touch every
    entry of V, against one tridiagonal reduction).  Measured over the 18 cases: residual 3.4e-15 worst (d = 128) against
    LAPACK's worst 1.3e-15; defect 2.9e-13 worst (d = 128, n = 255) against LAPACK's worst 1.9e-14; the bounds are
    2.1e-14 and 3.1e-13."""
    t = table()
    worst_r, worst_o = max(v[2] for v in t.values()), max(v[3] for v in t.values())
    for name, (r, o, rl, ol, _, _) in t.items():
        print(f"{name:10s} residual {r:.3e} (LAPACK {rl:.3e})  defect {o:.3e} (LAPACK {ol:.3e})")
    print(f"LAPACK's worst: residual {worst_r:.3e}, defect {worst_o:.3e}")
    for name, (r, o, _, _, _, _) in t.items():
        assert r <= 16 * worst_r, (name, r, worst_r)
        assert o <= 16 * worst_o, (name, o, worst_o)


def test_eigenvalues_agree_within_weyls_bound():
    """|lambda_i - lambda_i'| <= (r_ref + r_lapack) |C|_F: each method's values are the exact ones of a matrix within its
    own residual of C (Weyl's inequality); no free number"""
    for name, (r, _, rl, _, norm, diff) in table().items():
        print(f"{name:10s} difference {diff:.3e}  bound {(r + rl) * norm:.3e}")
        assert diff <= (r + rl) * norm, (name, diff, (r + rl) * norm)


def test_the_covariance_is_the_direct_one():
    """the centred moments about an fp32 pivot against the two-pass fp64 covariance: a few rounding errors of the
    moments, n eps |x - p|^2 per entry at the most"""
    for case in R.CASES:
        Xl, s = solved(case[0])
        mean, C, _, _ = R.direct(Xl)
        n = Xl.shape[0]
        spread = (np.abs(Xl.astype(np.float64) - mean) ** 2).sum(0).max() / (n - 1)
        assert np.abs(s.cov - C).max() <= 4 * n * 2.0 ** -52 * max(spread, 1e-300), case[0]
        assert np.abs(s.mean - mean).max() <= 2.0 ** -50 * max(np.abs(mean).max(), 1.0), case[0]


def test_every_case_converges_below_the_cap():
    for case in R.CASES:
        _, s = solved(case[0])
        assert s.info == 0 and 1 <= s.n_sweeps < R.MAX_SWEEPS, (case[0], s.info, s.n_sweeps)
        assert s.off_norm <= 2.0 ** -40 * max(np.linalg.norm(s.cov), 1e-300), (case[0], s.off_norm)
    assert solved("d1")[1].n_sweeps == 1 and solved("d1")[1].n_rotations == 0


def test_ordering_ties_and_sign():
    """values descend; the entry of largest magnitude of every component is positive, ties to the lower index; isotropic
    data with rows +-e_i has all eigenvalues equal and gives the identity in index order without a rotation"""
    for case in R.CASES:
        _, s = solved(case[0])
        assert np.all(np.diff(s.all_values) <= 0), case[0]
        at = np.abs(s.all_components).argmax(1)
        assert np.all(s.all_components[np.arange(len(at)), at] > 0), case[0]
    d = 5
    X = np.concatenate([np.eye(d), -np.eye(d)]).astype(np.float32)
    s = R.solve(R.moments(X), d, 1, None, d)
    assert s.info == 0 and s.n_sweeps == 1 and s.n_rotations == 0
    assert np.array_equal(s.components, np.eye(d)) and np.array_equal(s.values, np.full(d, 2.0 / 9.0))
    assert np.array_equal(s.mean, np.zeros(d))
    # equal magnitudes inside one component: the lower index is the one made positive
    A = np.array([[1.0, -1.0], [-1.0, 1.0]])
    values, comps, _ = R.finish(*R.jacobi(A)[:2])
    assert np.array_equal(values, [2.0, 0.0]) and comps[0, 0] > 0 > comps[0, 1] and abs(comps[0, 0]) == abs(comps[0, 1])
    # equal eigenvalues: the lower index of the final diagonal first
    values, comps, _ = R.finish(np.diag([3.0, 5.0, 3.0]), np.eye(3))
    assert np.array_equal(values, [5.0, 3.0, 3.0]) and np.array_equal(comps, np.eye(3)[[1, 0, 2]])


def test_the_round_robin_meets_every_pair_once():
    for dp in (2, 4, 18, 128):
        seen = set()
        for r in range(dp - 1):
            ps = R.pairs(dp, r)
            assert sorted(i for p in ps for i in p) == list(range(dp))           # disjoint, nobody left out
            seen |= set(ps)
        assert len(seen) == dp * (dp - 1) // 2


def test_too_few_rows_and_the_transform():
    X = np.array([[1.0, 2.0]], np.float32)
    s = R.solve(R.moments(X), 2, 1, None, 2)
    assert s.info == -1 and np.isnan(s.values).all() and np.isnan(s.components).all() and np.isnan(s.mean).all()
    Xl, s = solved("d17")
    Z = R.transform(Xl, s.mean, s.components[:3])
    Z64 = (Xl.astype(np.float64) - s.mean) @ s.components[:3].T
    bound = (17 + 2) * 2.0 ** -24 * (np.abs(Xl.astype(np.float64) - s.mean) @ np.abs(s.components[:3].T))
    assert Z.dtype == np.float32 and np.all(np.abs(Z - Z64) <= bound)
    lam = np.array([4.0, 0.0, -1e-20])
    Zw = R.transform(Xl, s.mean, s.components[:3], lam, whiten=True)
    assert np.array_equal(Zw[:, 0], Z[:, 0] * np.float32(0.5)) and not Zw[:, 1:].any()
    Xl = Xl.copy()
    Xl[4, 2] = np.inf
    Zb = R.transform(Xl, s.mean, s.components[:3])
    assert np.isnan(Zb[4]).all() and np.array_equal(Zb[5:], Z[5:])


# ------------------------------------------------------------------------------------------------ the C ABI, no GPU
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    return _lib.load()


def test_workspace_is_a_pure_function_of_d(lib):
    sizes = [lib.gae_pca_workspace_bytes(d) for d in range(1, 129)]
    assert all(s >= d * d * 8 and s > 0 for d, s in zip(range(1, 129), sizes))
    assert sizes == [lib.gae_pca_workspace_bytes(d) for d in range(1, 129)] and sizes == sorted(sizes)
    for d in (0, -1, 129, 2 ** 40):
        assert lib.gae_pca_workspace_bytes(d) == GAE_E_RANGE
    assert b"outside 1..128" in lib.gae_last_error()


def test_solve_argument_errors_need_no_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    need = lib.gae_pca_workspace_bytes(16)

    def solve(stats=p, d=16, t=1, pivot=None, n_used=100, k=2, flags=0, mean=p, values=p, comps=p, status=p, ws=p, nbytes=need):
        return lib.gae_pca_solve(stats, d, t, pivot, n_used, k, flags, mean, values, comps, status, ws, nbytes, None)
    assert solve(d=0) == GAE_E_RANGE and solve(d=129) == GAE_E_RANGE and b"outside 1..128" in lib.gae_last_error()
    assert solve(k=0) == GAE_E_RANGE and solve(k=17) == GAE_E_RANGE and b"n_components" in lib.gae_last_error()
    assert solve(t=-1) == GAE_E_RANGE and solve(t=9) == GAE_E_RANGE
    assert solve(flags=1) == GAE_E_RANGE and b"unknown flags" in lib.gae_last_error()
    assert solve(n_used=-1) == GAE_E_SIZE and solve(n_used=2 ** 31) == GAE_E_SIZE
    for name in ("stats", "mean", "values", "comps", "status", "ws"):
        assert solve(**{name: None}) == GAE_E_NULL, name
    assert solve(nbytes=need - 1) == GAE_E_WORKSPACE and b"needed" in lib.gae_last_error()


def test_transform_argument_errors_need_no_gpu(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def transform(X=p, ldx=16, n=10, d=16, rows=None, n_rows=10, mean=p, comps=p, values=None, k=2, flags=0, Z=p, ldz=2,
                  status=p):
        return lib.gae_pca_transform(X, ldx, n, d, rows, n_rows, mean, comps, values, k, flags, Z, ldz, status, None)
    assert transform(d=0) == GAE_E_RANGE and transform(d=129, ldx=129) == GAE_E_RANGE
    assert transform(k=0) == GAE_E_RANGE and transform(k=17, ldz=17) == GAE_E_RANGE
    assert transform(flags=2) == GAE_E_RANGE and b"unknown flags" in lib.gae_last_error()
    assert transform(n=-1) == GAE_E_SIZE and transform(n_rows=-1, rows=p) == GAE_E_SIZE
    assert transform(n=2 ** 31, n_rows=2 ** 31) == GAE_E_SIZE
    assert transform(ldx=15) == GAE_E_SIZE and transform(ldz=1) == GAE_E_SIZE
    assert transform(n_rows=5) == GAE_E_SIZE and b"rows is NULL" in lib.gae_last_error()
    for name in ("X", "Z", "mean", "comps", "status"):
        assert transform(**{name: None}) == GAE_E_NULL, name
    assert transform(flags=1) == GAE_E_NULL and b"WHITEN" in lib.gae_last_error()
    assert transform(n=0, n_rows=0, X=None, Z=None) == 0                     # nothing to do: no launch
