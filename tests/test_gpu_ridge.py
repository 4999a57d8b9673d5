"""K25 on the device (gae_ridge_stats, gae_ridge_solve, ops.ridge, GAE.ridge_graphs, the embed script) against the fp64
restatement tests/ridge_ref.py.  Shapes are the smallest at which each mechanism can break: one product of four rows and
its tails (n = 1, 3, 4, 5), a stage of 32 rows and two (63, 64, 65), one chunk of C = RIDGE_CHUNK_ROWS rows and its
neighbours (C - 1, C, C + 1, 2 C + 3), a list of more than 32 chunks (the 64-lane order of the partial sums), every
tile count of the padded width (d = 1 .. 128 with t = 1, 3, 8), one fold, several, and more folds than rows."""
import functools

import numpy as np
import pytest
import torch

import ridge_ref as R
from gae_dgl_amd._lib import RIDGE_CHUNK_ROWS
from ridge_ref import LAMBDAS, bound_of, errors_over_bound, make_case

pytestmark = pytest.mark.gpu
NAN = float("nan")
C = RIDGE_CHUNK_ROWS
CANARY = 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    from gae_dgl_amd import ops
    assert ops.RIDGE_CHUNK_ROWS == C
    return torch.device("cuda:0")


def as_np(t):
    return t.detach().cpu().numpy()


def strided(X, pad, dev):
    """X [n, w] on the device as a view of a [n, w + pad] buffer whose pad columns hold NaN: never read as data"""
    X = torch.as_tensor(X, dtype=torch.float32)
    buf = torch.full((X.shape[0], X.shape[1] + pad), NAN, dtype=torch.float32)
    buf[:, :X.shape[1]] = X
    return buf.to(dev)[:, :X.shape[1]]


def raw_stats(X, Y, pivot, rows, fold_ptr, F, n_rows=None):
    """gae_ridge_stats on device tensors (strided views allowed).  stats and the workspace are followed by canaries that
    must come back untouched.  Returns (stats fp64 [F, tri(W)] on the host, status int64 [4])"""
    from gae_dgl_amd import _lib
    from gae_dgl_amd.ops import _ptr, _stream
    n, d = X.shape
    t = Y.shape[1]
    dv = X.device
    ldx = X.stride(0) if n > 1 else d
    ldy = Y.stride(0) if n > 1 else t
    if n_rows is None:
        n_rows = n if rows is None else rows.shape[0]
    nbytes = _lib.load().gae_ridge_workspace_bytes(n_rows, d, t, F)
    assert nbytes > 0
    ws = torch.full((nbytes + CANARY,), 0xA5, dtype=torch.uint8, device=dv)
    size = F * R.tri(1 + d + t)
    stats = torch.full((size + CANARY,), -7.0, dtype=torch.float64, device=dv)
    status = torch.zeros(4, dtype=torch.int64, device=dv)
    pv = None if pivot is None else torch.as_tensor(pivot, dtype=torch.float32).to(dv)
    _lib.call("gae_ridge_stats", _ptr(X), ldx, _ptr(Y), ldy, n, d, t, _ptr(pv), _ptr(rows), n_rows, _ptr(fold_ptr), F,
              _ptr(stats), _ptr(status), _ptr(ws), nbytes, _stream())
    torch.cuda.synchronize()
    assert bool((stats[size:] == -7.0).all()), "a store beyond stats"
    assert bool((ws[nbytes:] == 0xA5).all()), "a store beyond the workspace"
    return as_np(stats[:size]).reshape(F, -1), as_np(status)


def raw_solve(stats, d, t, lambdas, pivot, flags, dev):
    from gae_dgl_amd import _lib
    from gae_dgl_amd.ops import _ptr, _stream
    F, L = stats.shape[0], len(lambdas)
    st = torch.from_numpy(stats).to(dev)
    lam = torch.tensor(lambdas, dtype=torch.float64, device=dev)
    pv = None if pivot is None else torch.as_tensor(pivot, dtype=torch.float32).to(dev)
    coef = torch.full(((F + 1) * L * t * d + CANARY,), -7.0, dtype=torch.float64, device=dev)
    icpt = torch.full(((F + 1) * L * t + CANARY,), -7.0, dtype=torch.float64, device=dev)
    sse = torch.full((F * L * t + CANARY,), -7.0, dtype=torch.float64, device=dev)
    info = torch.full(((F + 1) * L + CANARY,), -7, dtype=torch.int32, device=dev)
    status = torch.zeros(4, dtype=torch.int64, device=dev)
    _lib.call("gae_ridge_solve", _ptr(st), d, t, F, _ptr(pv), _ptr(lam), L, flags, _ptr(coef), _ptr(icpt), _ptr(sse),
              _ptr(info), _ptr(status), _stream())
    torch.cuda.synchronize()
    for buf in (coef, icpt, sse, info):
        assert bool((buf[-CANARY:] == -7).all()), "a store beyond an output"
    return (as_np(coef[:-CANARY]).reshape(F + 1, L, t, d), as_np(icpt[:-CANARY]).reshape(F + 1, L, t),
            as_np(sse[:-CANARY]).reshape(F, L, t), as_np(info[:-CANARY]).reshape(F + 1, L), as_np(status))


def grid(rng, n, w):
    """multiples of 1/4 in [-4, 4]: with a pivot of the same kind v lies in [-8, 8], every product is a multiple of 1/16
    below 2^6 and every sum of up to 2^16 of them is exact in fp64, in any order"""
    return (rng.integers(-16, 17, (n, w)) / 4.0).astype(np.float32)


# ------------------------------------------------------------------ 1. the moments, bit for bit on an exact grid
NS = [1, 3, 4, 5, 63, 64, 65, C - 1, C, C + 1, 2 * C + 3]
DS, TS, FS = [1, 15, 16, 17, 48, 127, 128], [1, 3, 8], [1, 2, 5, 32]
GRID_CASES = sorted({(NS[i % 11], DS[i % 7], TS[i % 3], FS[(i // 2) % 4]) for i in range(22)}
                    | {(2 * C + 3, 128, 8, 5), (C + 1, 127, 8, 32), (65, 48, 1, 5), (33 * C + 5, 17, 1, 2)})


def test_the_grid_cases_cover_every_value_of_every_axis():
    for axis, values in enumerate((NS, DS, TS, FS)):
        assert set(values) <= {c[axis] for c in GRID_CASES}
    assert any(n > 32 * C for n, _, _, _ in GRID_CASES)                 # the 64-lane order of the chunk partials


@pytest.mark.parametrize("n, d, t, F", GRID_CASES)
def test_stats_exact_on_a_grid(dev, n, d, t, F):
    """strided X / Y whose pad columns hold NaN, unlisted rows (fold -1) filled with NaN, a non-zero pivot"""
    rng = np.random.default_rng(n * 1000003 + d * 1009 + t * 17 + F)
    X, Y, pivot = grid(rng, n, d), grid(rng, n, t), grid(rng, 1, d + t)[0]
    if n > 32 * C:
        fold = np.where(np.arange(n) < 7, 1, 0)                        # 33 chunks and a tail in fold 0, 7 rows in fold 1
    else:
        fold = rng.integers(-1, F, n)
    fold[rng.integers(0, n)] = 0                                       # at least one listed row
    X[fold < 0] = NAN
    Y[fold < 0] = NAN
    rows, fold_ptr = R.fold_lists(fold, F)
    want = R.moments(X, Y, rows, fold_ptr, pivot)
    got, status = raw_stats(strided(X, 3, dev), strided(Y, 2, dev), pivot, torch.from_numpy(rows).to(dev),
                            torch.from_numpy(fold_ptr).to(dev), F)
    assert status.tolist() == [0, 0, 0, 0]
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    for f in range(F):
        if fold_ptr[f] == fold_ptr[f + 1]:
            assert not got[f].any()                                    # a fold without rows: an all-zero block


def test_a_fold_without_rows_and_rows_that_no_fold_owns(dev):
    rng = np.random.default_rng(3)
    n, d, t, F = 70, 5, 2, 4
    X, Y = grid(rng, n, d), grid(rng, n, t)
    fold = rng.integers(0, F, n)
    fold[fold == 2] = -1                                               # fold 2 is empty
    X[fold < 0] = NAN
    rows, fold_ptr = R.fold_lists(fold, F)
    assert fold_ptr[2] == fold_ptr[3]
    got, status = raw_stats(torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev), None,
                            torch.from_numpy(rows).to(dev), torch.from_numpy(fold_ptr).to(dev), F)
    assert status.tolist() == [0, 0, 0, 0]
    assert np.array_equal(got, R.moments(X, Y, rows, fold_ptr)) and not got[2].any() and got[0].any()


def test_a_fold_shorter_than_a_chunk_between_two_longer_ones_and_no_row_list(dev):
    """folds of C + 1, 7 and C + 5 rows: chunks 0-1, 2 and 3-4 of a grid of cdiv(2 C + 13, C) + 3 = 6 blocks, the last one
    spare; then the same rows without a list (rows == NULL: one fold; that grid is cdiv(n, C) blocks and has no spare
    one).  Exact as the grid cases"""
    rng = np.random.default_rng(11)
    n, d, t, F = 2 * C + 13 + 9, 17, 3, 3
    X, Y, pivot = grid(rng, n, d), grid(rng, n, t), grid(rng, 1, d + t)[0]
    fold = np.full(n, -1)
    listed = rng.permutation(n)[:2 * C + 13]                           # 9 rows are left out
    fold[listed[:C + 1]], fold[listed[C + 1:C + 8]], fold[listed[C + 8:]] = 0, 1, 2
    X[fold < 0] = NAN
    Y[fold < 0] = NAN
    rows, fold_ptr = R.fold_lists(fold, F)
    assert np.diff(fold_ptr).tolist() == [C + 1, 7, C + 5]
    got, status = raw_stats(strided(X, 3, dev), strided(Y, 2, dev), pivot, torch.from_numpy(rows).to(dev),
                            torch.from_numpy(fold_ptr).to(dev), F)
    assert status.tolist() == [0, 0, 0, 0]
    want = R.moments(X, Y, rows, fold_ptr, pivot)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    Xl, Yl = X[fold >= 0], Y[fold >= 0]
    got, status = raw_stats(strided(Xl, 3, dev), strided(Yl, 2, dev), pivot, None, None, 1)
    assert status.tolist() == [0, 0, 0, 0]
    want = R.moments(Xl, Yl, None, None, pivot)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert np.array_equal(got[0], R.moments(X, Y, rows, fold_ptr, pivot).sum(0))       # exact sums: the folds add up


# ------------------------------------------------------------------ 2. the same bits
@pytest.mark.parametrize("n, d, t", [(2 * C + 3, 48, 1), (33 * C + 5, 16, 2)])
def test_same_bits_run_to_run_for_any_stride_and_through_the_row_list(dev, n, d, t):
    rng = np.random.default_rng(n)
    X, Y = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((n, t)).astype(np.float32)
    pivot = np.concatenate([X.mean(0), Y.mean(0)]).astype(np.float32)
    Xd, Yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
    base, _ = raw_stats(Xd, Yd, pivot, None, None, 1)
    assert np.isfinite(base).all()
    runs = [raw_stats(Xd, Yd, pivot, None, None, 1)[0],                                            # again
            raw_stats(strided(X, 7, dev), strided(Y, 1, dev), pivot, None, None, 1)[0],            # other strides
            raw_stats(Xd, Yd, pivot, torch.arange(n, dtype=torch.int32, device=dev),              # the list 0 .. n - 1
                      torch.tensor([0, n], dtype=torch.int32, device=dev), 1)[0]]
    with torch.cuda.stream(torch.cuda.Stream()):
        runs.append(raw_stats(Xd, Yd, pivot, None, None, 1)[0])                                    # another stream
    for r in runs:
        assert np.array_equal(r.view(np.int64), base.view(np.int64))
    # n terms per entry, each sum's worst case n eps sum |terms| <= n eps max(diagonal), once for each of the two routes
    want = R.moments(X, Y, None, None, pivot)
    assert np.abs(base - want).max() <= 2 * n * 2.0 ** -53 * np.abs(want).max()


# ------------------------------------------------------------------ 3. the models, inside the derived bound
SOLVE_CASES = [(300, 48, 1, 5, 0.0, "mean"), (40, 48, 3, 2, 0.0, "mean"), (65, 128, 8, 3, 0.0, "mean"),
               (1000, 16, 2, 5, 1e3, "mean"), (1000, 16, 2, 5, 1e3, None)]


@functools.lru_cache(maxsize=None)
def reference(n, d, t, F, offset, pivot):
    """computed once per case and shared: the data, the direct route's tables, the bound per (model, lambda)"""
    X, Y, fold = make_case(n, d, t, F, offset)
    p = np.concatenate([X.mean(0), Y.mean(0)]).astype(np.float32) if pivot == "mean" else None
    coef, icpt, sse, cond = R.direct(X, Y, fold, LAMBDAS)
    Yd = Y.astype(np.float64)
    sst = ((Yd - Yd.mean(0)) ** 2).sum(0)
    return X, Y, fold, p, (coef, icpt, sse), sst, bound_of(X, Y, fold, F, p, cond)


@pytest.mark.parametrize("n, d, t, F, offset, pivot", SOLVE_CASES)
def test_solve_against_the_reference_from_the_same_stats(dev, n, d, t, F, offset, pivot):
    """|dw|_inf / |w|_inf and |dSSE| / SST <= 64 d kappa (1 + rho^2) 2^-53, kappa = cond(C_xx + lambda I) of the reference,
    rho = max_f |mean_f - pivot| / std_f"""
    X, Y, fold, p, direct, sst, bound = reference(n, d, t, F, offset, pivot)
    rows, fold_ptr = R.fold_lists(fold, F)
    stats, status = raw_stats(torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev), p, torch.from_numpy(rows).to(dev),
                              torch.from_numpy(fold_ptr).to(dev), F)
    assert status.tolist() == [0, 0, 0, 0]
    coef, icpt, sse, info, status = raw_solve(stats, d, t, LAMBDAS, p, 0, dev)
    want = R.solve(stats, d, t, LAMBDAS, p)
    assert status.tolist() == [0, 0, 0, 0] and (info == 0).all() and (want[3] == 0).all()
    for name, ref in (("solve()", want[:3]), ("direct()", direct)):
        ew, es, eb = errors_over_bound((coef, icpt, sse), ref, sst, bound, X, Y)
        print(f"against {name}: coef error / bound = {ew:.3g}, SSE error / bound = {es:.3g}, intercept / limit = {eb:.3g}")
        assert ew <= 1.0 and es <= 1.0 and eb <= 1.0


@pytest.mark.parametrize("n, d, t, F, offset, pivot", SOLVE_CASES)
def test_ops_ridge_end_to_end_against_the_direct_route(dev, n, d, t, F, offset, pivot):
    from gae_dgl_amd import ops
    X, Y, fold, p, (coef, icpt, sse), sst, bound = reference(n, d, t, F, offset, pivot)
    res = ops.ridge(torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev), folds=F, fold=torch.from_numpy(fold).to(dev),
                    pivot=pivot)
    assert res.n_used == n and res.fold_counts.tolist() == [int((fold == f).sum()) for f in range(F)]
    assert res.coef.shape == (t, d) and res.coef.dtype == torch.float64 and res.intercept.shape == (t,)
    assert as_np(res.lambdas).tolist() == LAMBDAS and not as_np(res.info).any()
    # of the F + 1 models the result carries the all-rows one (path_*): the folds' own rows stand in for the others
    got = (np.concatenate([coef[:F], as_np(res.path_coef)[None]]), np.concatenate([icpt[:F], as_np(res.path_intercept)[None]]),
           as_np(res.cv_sse))
    ew, es, eb = errors_over_bound(got, (coef, icpt, sse), sst, bound, X, Y)
    print(f"coef error / bound = {ew:.3g}, SSE error / bound = {es:.3g}, intercept error / limit = {eb:.3g}")
    assert ew <= 1.0 and es <= 1.0 and eb <= 1.0
    pooled = sse.sum(0)
    r2 = 1 - pooled / sst
    # the pooled SSE is within F bound SST of the reference's: so is R2 (in units of 1) and the squared RMSE (of SST / n)
    tol = F * bound[:F].max(0)[:, None]
    assert (np.abs(as_np(res.cv_r2) - r2) <= tol).all()
    assert (np.abs(as_np(res.cv_rmse) ** 2 - pooled / n) <= tol * sst / n).all()
    chosen = int(np.argmin((1 - r2).mean(1)))
    assert res.lam == LAMBDAS[chosen]
    assert torch.equal(res.coef, res.path_coef[chosen]) and torch.equal(res.intercept, res.path_intercept[chosen])


# ------------------------------------------------------------------ 4. failure paths that are results, not faults
def test_a_duplicated_column_fails_at_lambda_zero_and_is_never_chosen(dev):
    """+-1 columns over 9 / 16 / 25 training rows, no intercept, no pivot: sqrt and the division are exact, so the second
    column of the pair meets a pivot of exactly 0.0 in every model (tests/test_ridge_cpu.py shows the same in numpy)"""
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    rng = np.random.default_rng(1)
    X = rng.choice([-1.0, 1.0], (25, 3)).astype(np.float32)
    X[:, 1] = X[:, 0]
    y = rng.standard_normal(25).astype(np.float32)
    fold = torch.tensor([0] * 16 + [1] * 9, device=dev)
    Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
    res = ops.ridge(Xd, yd, [0.0, 0.5], folds=2, fold=fold, fit_intercept=False, pivot=None)
    assert as_np(res.info).tolist() == [[2, 0], [2, 0], [2, 0]]
    assert res.lam == 0.5 and bool(torch.isfinite(res.coef).all())
    assert bool(torch.isnan(res.path_coef[0]).all()) and bool(torch.isnan(res.path_intercept[0]).all())
    assert bool(torch.isnan(res.cv_sse[:, 0]).all()) and bool(torch.isfinite(res.cv_sse[:, 1]).all())
    assert bool(torch.isnan(res.cv_r2[0]).all())
    with pytest.raises(GaeHipError, match="none of the 1 lambdas"):
        ops.ridge(Xd, yd, [0.0], folds=2, fold=fold, fit_intercept=False, pivot=None)


def test_non_finite_listed_rows_raise_with_their_count(dev):
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    X, y = torch.randn(200, 8, device=dev), torch.randn(200, device=dev)
    fold = torch.arange(200, device=dev) % 4
    fold[[5, 6]] = -1
    Xb, yb = X.clone(), y.clone()
    Xb[5] = NAN                                                        # left out: never read
    assert ops.ridge(Xb, yb, folds=4, fold=fold).n_used == 198
    Xb[10, 3] = NAN; Xb[10, 4] = float("inf"); Xb[77, 0] = -float("inf"); yb[150] = NAN      # three listed rows
    for pivot in ("mean", None):
        with pytest.raises(GaeHipError, match="3 of the 198 listed rows hold non-finite values"):
            ops.ridge(Xb, yb, folds=4, fold=fold, pivot=pivot)


def test_bad_fold_lists_and_lambdas_are_reported_through_the_status_block(dev):
    from gae_dgl_amd import _lib
    rng = np.random.default_rng(9)
    n, d, t = 50, 4, 1
    X, Y = torch.from_numpy(grid(rng, n, d)).to(dev), torch.from_numpy(grid(rng, n, t)).to(dev)
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    for fp in ([0, 30, 20, 50], [0, 20, 30, 49], [0, 20, 30, 2 ** 31 - 1], [-5, 20, 30, 50]):      # not monotone; last != n_rows
        got, status = raw_stats(X, Y, None, rows, torch.tensor(fp, dtype=torch.int32, device=dev), 3)
        assert status.tolist() == [0, _lib.RIDGE_ERR_FOLD_PTR, 0, 0], fp
        assert np.isnan(got).all()
    bad_rows = rows.clone()
    bad_rows[7], bad_rows[40] = n, -1                                  # ids outside [0, n): flagged and skipped
    got, status = raw_stats(X, Y, None, bad_rows, torch.tensor([0, 20, 30, 50], dtype=torch.int32, device=dev), 3)
    assert status.tolist() == [0, _lib.RIDGE_ERR_ROW_ID, 0, 0]
    keep = np.array([r for r in range(n) if r not in (7, 40)], dtype=np.int32)
    assert np.array_equal(got, R.moments(as_np(X), as_np(Y), keep, np.array([0, 19, 29, 48])))
    stats = R.moments(as_np(X), as_np(Y), None, None)
    coef, icpt, sse, info, status = raw_solve(stats, d, t, [1.0, -1.0, float("nan"), float("inf")], None, 0, dev)
    assert status.tolist() == [0, _lib.RIDGE_ERR_LAMBDA, 0, 0]
    assert info.tolist() == [[-1, -2, -2, -2], [0, -2, -2, -2]]       # model 0 of one fold trains on nothing
    assert np.isfinite(coef[1, 0]).all() and np.isnan(coef[0]).all() and np.isnan(coef[1, 1:]).all() and np.isnan(sse).all()


def test_equal_lambdas_one_fold_and_no_intercept(dev):
    from gae_dgl_amd import ops
    X, Y, fold = make_case(300, 12, 2, 3, 0.5)
    Xd, Yd, fd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev), torch.from_numpy(fold).to(dev)
    tie = ops.ridge(Xd, Yd, [2.0, 2.0, 2.0], folds=3, fold=fd)          # equal scores: the lower index
    assert tie.lam == 2.0 and torch.equal(tie.cv_r2[0], tie.cv_r2[2]) and torch.equal(tie.coef, tie.path_coef[0])
    # folds = 1: the plain fit on all rows, against the normal equations in numpy
    one = ops.ridge(Xd, Yd, [2.0], folds=1)
    Xc, Yc = X.astype(np.float64) - X.astype(np.float64).mean(0), Y.astype(np.float64) - Y.astype(np.float64).mean(0)
    w = np.linalg.solve(Xc.T @ Xc + 2.0 * np.eye(12), Xc.T @ Yc).T
    assert one.n_used == 300 and one.lam == 2.0 and one.fold_counts.tolist() == [300]
    assert np.allclose(as_np(one.coef), w, rtol=1e-10, atol=1e-12)
    assert np.allclose(as_np(one.coef), as_np(tie.coef), rtol=1e-10, atol=1e-12)
    assert bool(torch.isnan(one.cv_r2).all())
    # fit_intercept = False, with and without a pivot
    coef, icpt, sse, _ = R.direct(X, Y, fold, LAMBDAS, fit_intercept=False)
    for pivot in ("mean", None):
        res = ops.ridge(Xd, Yd, folds=3, fold=fd, fit_intercept=False, pivot=pivot)
        assert not as_np(res.intercept).any() and not as_np(res.path_intercept).any()
        assert np.allclose(as_np(res.path_coef), coef[3], rtol=1e-9, atol=1e-12)
        assert np.allclose(as_np(res.cv_sse), sse, rtol=1e-9)
    with pytest.raises(ValueError, match="holds no rows"):
        ops.ridge(Xd, Yd, folds=4, fold=fd)
    with pytest.raises(ValueError):
        ops.ridge(Xd, Yd, folds=2, fold=fd)                             # a value beyond folds - 1


# ------------------------------------------------------------------ 5. the surface
def test_ridge_graphs_is_ridge_of_the_molecule_features(dev):
    import gae_dgl_amd as G
    from gae_dgl_amd import ops
    from gae_dgl_amd.dataset import DeviceGraphDataset
    data = DeviceGraphDataset.synthetic_zinc(600, seed=1, device=dev)
    torch.manual_seed(0)
    model = G.GAE(39, [32, 16]).to(dev).eval()
    y = torch.randn(600, 2, generator=torch.Generator().manual_seed(2)).to(dev)
    feats = model.embed_graphs(data)
    want = ops.ridge(feats, y, folds=4, seed=3)
    res = model.ridge_graphs(data, y, folds=4, seed=3, fused="auto", batch_size=256)
    for a, b in zip(res, want):
        if isinstance(a, torch.Tensor):
            assert torch.equal(a, b)
        else:
            assert a == b
    assert res.coef.shape == (2, 48) and res.n_used == 600
    with pytest.raises(ValueError):
        model.ridge_graphs(data, y, grad=True)


def test_predict_reproduces_targets_that_are_linear_in_the_features(dev):
    """X on the 1/4 grid, w and b small multiples of 1/4: y = X w + b is exact in fp32.  With lambda = 0 the only error is
    the solve's: |dw|_inf <= B |w|_inf with the bound B of group 3, so |predict(x) - y| <= B |w|_inf |x - mean|_1 plus the
    rounding of the intercept and of the product itself (8 eps |y|)"""
    from gae_dgl_amd import ops
    rng = np.random.default_rng(5)
    n, d, t, F = 400, 10, 2, 5
    X = grid(rng, n, d)
    w = rng.integers(-8, 9, (t, d)) / 4.0
    b = np.array([0.75, -2.5])
    Yx = X.astype(np.float64) @ w.T + b
    Y = Yx.astype(np.float32)
    assert np.array_equal(Y.astype(np.float64), Yx)
    fold = rng.permutation(n) % F
    Xd = torch.from_numpy(X).to(dev)
    res = ops.ridge(Xd, torch.from_numpy(Y).to(dev), [0.0], folds=F, fold=torch.from_numpy(fold).to(dev))
    Xc = X.astype(np.float64) - X.astype(np.float64).mean(0)
    p = np.concatenate([X.mean(0), Y.mean(0)]).astype(np.float32)
    B = float(np.max(bound_of(X, Y, fold, F, p, np.linalg.cond(Xc.T @ Xc))))
    assert np.abs(as_np(res.coef) - w).max() <= B * np.abs(w).max()
    err = np.abs(as_np(res.predict(Xd)) - Yx).max()
    limit = B * np.abs(w).max() * np.abs(Xc).sum(1).max() + 8 * 2.0 ** -53 * np.abs(Yx).max()
    print(f"max |predict - y| = {err:.3g}, limit {limit:.3g}")
    assert err <= limit
    # the targets have no residual: the pooled SSE is its own error, at most F B SST
    assert float(res.cv_r2.min()) >= 1 - F * B and float(res.cv_rmse.max()) <= np.sqrt(F * B * Yx.var(0).max())


def test_cli_embed_ridge(tmp_path, capsys):
    from gae_dgl_amd import embed as E
    import gae_dgl_amd as G
    torch.manual_seed(0)
    ckpt = str(tmp_path / "m.pkl")
    torch.save(G.GAE(39, [32, 16]).state_dict(), ckpt)
    ng = 300
    y = np.random.default_rng(1).standard_normal((ng, 2))
    np.save(tmp_path / "y.npy", y)
    E.main(["--checkpoint", ckpt, "--hidden_dims", "32", "16", "--synthetic", str(ng), "--out", str(tmp_path / "f.npy"),
            "--ridge", "0.1", "10", "1000", "--ridge_folds", "3", "--ridge_out", str(tmp_path / "model.npz"),
            "--targets", str(tmp_path / "y.npy")])
    text = capsys.readouterr().out
    assert f"Fitted ridge on {ng} molecules, 3 lambdas x 3 folds" in text
    line = [l for l in text.splitlines() if l.startswith("Ridge (3-fold CV, lambda = ")]
    assert len(line) == 1 and line[0].count("RMSE:") == 2 and line[0].count("R2:") == 2, text
    z = np.load(tmp_path / "model.npz")
    res = E.main.ridge
    assert sorted(z.files) == ["coef", "cv_r2", "cv_rmse", "intercept", "lam", "lambdas"]
    assert z["coef"].shape == (2, 48) and z["coef"].dtype == np.float64 and z["lambdas"].tolist() == [0.1, 10.0, 1000.0]
    assert np.array_equal(z["coef"], as_np(res.coef)) and np.array_equal(z["intercept"], as_np(res.intercept))
    assert float(z["lam"]) == res.lam and np.array_equal(z["cv_rmse"], as_np(res.cv_rmse))
    chosen = z["lambdas"].tolist().index(float(z["lam"]))
    assert f"lambda = {res.lam:g})" in line[0]
    nums = [float(v) for v in line[0].split(") ")[1].replace("RMSE: ", "").replace("R2: ", "").split(" | ")]
    assert nums == pytest.approx([z["cv_rmse"][chosen, 0], z["cv_r2"][chosen, 0], z["cv_rmse"][chosen, 1],
                                  z["cv_r2"][chosen, 1]], abs=2e-6)
    # the saved model predicts like the result
    feats = np.load(tmp_path / "f.npy").astype(np.float64)
    assert np.allclose(feats @ z["coef"].T + z["intercept"], as_np(res.predict(E.main.features)), rtol=1e-12, atol=1e-12)
