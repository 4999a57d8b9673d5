"""K25 without a GPU: the fp64 restatement tests/ridge_ref.py (its moment route against its direct route, inside the bound
the GPU tests use), the argument errors of gae_ridge_stats / gae_ridge_solve / gae_ridge_workspace_bytes (returned
before anything is dereferenced), the option checks of ops.ridge and the argument checks of the embed command line."""
import re
import os

import numpy as np
import pytest
import torch

import ridge_ref as R

E_NULL, E_SIZE, E_WORKSPACE, E_RANGE = -1, -2, -5, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMBDAS, make_case, bound_of, errors_over_bound = R.LAMBDAS, R.make_case, R.bound_of, R.errors_over_bound


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------ the reference: moments + solve against direct
CASES = [(300, 48, 1, 5, 0.0, "mean"), (40, 48, 3, 2, 0.0, "mean"), (65, 128, 8, 3, 0.0, "mean"),
         (1000, 16, 2, 5, 1e3, "mean"), (1000, 16, 2, 5, 1e3, None)]


@pytest.mark.parametrize("n, d, t, F, offset, pivot", CASES)
def test_moment_route_agrees_with_the_direct_route(n, d, t, F, offset, pivot):
    X, Y, fold = make_case(n, d, t, F, offset)
    rows, fold_ptr = R.fold_lists(fold, F)
    p = np.concatenate([X.mean(0), Y.mean(0)]).astype(np.float32) if pivot == "mean" else None
    stats = R.moments(X, Y, rows, fold_ptr, p)
    assert stats.shape == (F, R.tri(1 + d + t))
    coef, icpt, sse, info = R.solve(stats, d, t, LAMBDAS, p)
    coef2, icpt2, sse2, cond = R.direct(X, Y, fold, LAMBDAS)
    assert (info == 0).all()
    Yd = Y.astype(np.float64)
    sst = ((Yd - Yd.mean(0)) ** 2).sum(0)
    ew, es, eb = errors_over_bound((coef, icpt, sse), (coef2, icpt2, sse2), sst, bound_of(X, Y, fold, F, p, cond), X, Y)
    print(f"coef error / bound = {ew:.3g}, SSE error / bound = {es:.3g}, intercept error / limit = {eb:.3g}")
    assert ew <= 1.0 and es <= 1.0 and eb <= 1.0


def test_reference_without_intercept_and_its_failure_codes():
    X, Y, fold = make_case(200, 6, 2, 4, 0.5)
    rows, fold_ptr = R.fold_lists(fold, 4)
    p = np.concatenate([X.mean(0), Y.mean(0)]).astype(np.float32)
    want = R.direct(X, Y, fold, [0.0, 1.0], fit_intercept=False)
    for pivot in (None, p):                                            # the model does not depend on the pivot
        coef, icpt, sse, info = R.solve(R.moments(X, Y, rows, fold_ptr, pivot), 6, 2, [0.0, 1.0], pivot, R.NO_INTERCEPT)
        assert (info == 0).all() and (icpt == 0).all()
        assert np.allclose(coef, want[0], rtol=1e-9, atol=1e-12) and np.allclose(sse, want[2], rtol=1e-9)
    # a duplicated column at lambda = 0: the second of the pair has a zero pivot; [+-1, +-1] columns over 9 / 16 / 25
    # training rows make every step exact (sqrt(9), sqrt(16), sqrt(25)), so the pivot is 0.0, not a rounding residue
    rng = np.random.default_rng(1)
    Xd = rng.choice([-1.0, 1.0], (25, 3)).astype(np.float32)
    Xd[:, 1] = Xd[:, 0]
    fold2 = np.array([0] * 16 + [1] * 9)
    rows, fold_ptr = R.fold_lists(fold2, 2)
    st = R.moments(Xd, Y[:25], rows, fold_ptr)
    coef, icpt, sse, info = R.solve(st, 3, 2, [0.0, 0.5], None, R.NO_INTERCEPT)
    assert info[:, 0].tolist() == [2, 2, 2] and (info[:, 1] == 0).all()
    assert np.isnan(coef[:, 0]).all() and np.isnan(sse[:, 0]).all() and np.isfinite(coef[:, 1]).all()
    # an empty training set, a negative lambda
    st1 = R.moments(X, Y, None, None)
    coef, icpt, sse, info = R.solve(st1, 6, 2, [1.0, -1.0])
    assert info.tolist() == [[-1, -2], [0, -2]] and np.isfinite(coef[1, 0]).all() and np.isnan(coef[0]).all()


# ------------------------------------------------------------------ the C ABI's argument errors
def stats_call(lib, *, X=1 << 20, ldx=8, Y=1 << 21, ldy=2, n=100, d=8, t=2, pivot=None, rows=1 << 22, n_rows=60,
               fold_ptr=1 << 23, folds=3, stats=1 << 24, status=1 << 25, ws=1 << 26, ws_bytes=1 << 30):
    """gae_ridge_stats with made-up non-NULL addresses: an argument error must return before any of them is touched"""
    rc = lib.gae_ridge_stats(X, ldx, Y, ldy, n, d, t, pivot, rows, n_rows, fold_ptr, folds, stats, status, ws, ws_bytes,
                             None)
    return rc, lib.gae_last_error().decode()


@pytest.mark.parametrize("kw, code, text", [
    (dict(d=0), E_RANGE, "d = 0 outside 1..128"),
    (dict(d=129, ldx=200), E_RANGE, "d = 129 outside 1..128"),
    (dict(t=0), E_RANGE, "t = 0 outside 1..8"),
    (dict(t=9, ldy=9), E_RANGE, "t = 9 outside 1..8"),
    (dict(folds=0), E_RANGE, "folds = 0 outside 1..32"),
    (dict(folds=33), E_RANGE, "folds = 33 outside 1..32"),
    (dict(n_rows=-1), E_SIZE, "negative n_rows = -1"),
    (dict(n_rows=1 << 31), E_SIZE, "beyond int32 row ids"),
    (dict(n=-1), E_SIZE, "negative n = -1"),
    (dict(n=1 << 31), E_SIZE, "beyond int32 row ids"),
    (dict(ldx=7), E_SIZE, "ldx 7 < d"),
    (dict(ldy=1), E_SIZE, "ldy 1 < t"),
    (dict(rows=None), E_SIZE, "rows is NULL"),
    (dict(rows=None, n_rows=100, folds=2), E_SIZE, "rows is NULL"),
    (dict(fold_ptr=None), E_NULL, "fold_ptr is NULL"),
    (dict(X=None), E_NULL, "X / Y is NULL"),
    (dict(Y=None), E_NULL, "X / Y is NULL"),
    (dict(stats=None), E_NULL, "stats / status is NULL"),
    (dict(status=None), E_NULL, "stats / status is NULL"),
    (dict(ws=None), E_NULL, "workspace is NULL"),
    (dict(ws_bytes=16), E_WORKSPACE, "workspace of 16 bytes"),
])
def test_stats_argument_errors_come_before_any_access(lib, kw, code, text):
    rc, msg = stats_call(lib, **kw)
    assert rc == code, (rc, msg)
    assert msg.startswith("gae_ridge_stats: ") and text in msg, msg


def solve_call(lib, *, stats=1 << 20, d=8, t=2, folds=3, pivot=None, lambdas=1 << 21, L=4, flags=0, coef=1 << 22,
               icpt=1 << 23, sse=1 << 24, info=1 << 25, status=1 << 26):
    rc = lib.gae_ridge_solve(stats, d, t, folds, pivot, lambdas, L, flags, coef, icpt, sse, info, status, None)
    return rc, lib.gae_last_error().decode()


@pytest.mark.parametrize("kw, code, text", [
    (dict(d=0), E_RANGE, "d = 0 outside 1..128"),
    (dict(d=129), E_RANGE, "d = 129 outside 1..128"),
    (dict(t=9), E_RANGE, "t = 9 outside 1..8"),
    (dict(folds=0), E_RANGE, "folds = 0 outside 1..32"),
    (dict(folds=33), E_RANGE, "folds = 33 outside 1..32"),
    (dict(L=0), E_RANGE, "n_lambdas = 0 outside 1..64"),
    (dict(L=65), E_RANGE, "n_lambdas = 65 outside 1..64"),
    (dict(flags=2), E_RANGE, "unknown flags 0x2"),
    (dict(stats=None), E_NULL, "stats / lambdas is NULL"),
    (dict(lambdas=None), E_NULL, "stats / lambdas is NULL"),
    (dict(coef=None), E_NULL, "is NULL"),
    (dict(icpt=None), E_NULL, "is NULL"),
    (dict(sse=None), E_NULL, "is NULL"),
    (dict(info=None), E_NULL, "is NULL"),
    (dict(status=None), E_NULL, "is NULL"),
])
def test_solve_argument_errors_come_before_any_access(lib, kw, code, text):
    rc, msg = solve_call(lib, **kw)
    assert rc == code, (rc, msg)
    assert msg.startswith("gae_ridge_solve: ") and text in msg, msg


def test_workspace_query_is_a_monotone_host_function(lib):
    q = lib.gae_ridge_workspace_bytes
    from gae_dgl_amd import ops
    C = ops.RIDGE_CHUNK_ROWS
    assert q(0, 1, 1, 1) > 0 and q(1000, 48, 1, 5) == q(1000, 48, 1, 5)
    for d, t, F in ((1, 1, 1), (48, 1, 5), (128, 8, 32)):
        prev = 0
        for n in (0, 1, C - 1, C, C + 1, 2 * C + 3, 19717, 249455, 10 ** 6, 2 ** 31 - 1):
            cur = q(n, d, t, F)
            assert cur >= prev > -1, (n, d, t, F)
            prev = cur
        W = 1 + d + t
        # a packed triangle per chunk, a chunk per RIDGE_CHUNK_ROWS rows and one more per fold: never n x anything
        assert q(249455, d, t, F) <= (249455 // C + 1 + F) * W * (W + 1) // 2 * 8 + 512
    assert q(10, 0, 1, 1) == E_RANGE and q(10, 129, 1, 1) == E_RANGE and q(10, 8, 9, 1) == E_RANGE
    assert q(10, 8, 1, 33) == E_RANGE and b"folds = 33" in lib.gae_last_error()
    assert q(-1, 8, 1, 1) == E_SIZE and q(1 << 31, 8, 1, 1) == E_SIZE


def test_the_chunk_constant_is_the_headers():
    from gae_dgl_amd import ops, _lib
    text = open(os.path.join(ROOT, "include", "gae_hip_experimental.h")).read()
    assert int(re.search(r"GAE_RIDGE_CHUNK_ROWS = (\d+)", text).group(1)) == ops.RIDGE_CHUNK_ROWS == _lib.RIDGE_CHUNK_ROWS
    assert (ops.RIDGE_MAX_D, ops.RIDGE_MAX_T, ops.RIDGE_MAX_FOLDS, ops.RIDGE_MAX_LAMBDAS) == (128, 8, 32, 64)


# ------------------------------------------------------------------ the wrapper and the command line
def test_ops_ridge_has_no_cpu_fallback_and_checks_its_options():
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    X, y = torch.randn(30, 4), torch.randn(30)
    with pytest.raises(GaeHipError):
        ops.ridge(X, y)                                                # CPU tensors
    for bad in (dict(folds=0), dict(folds=33), dict(folds=2.5), dict(folds=True), dict(lambdas=[]),
                dict(lambdas=[1.0] * 65), dict(lambdas=[-1.0]), dict(lambdas=[float("nan")]), dict(lambdas=[float("inf")]),
                dict(folds=1), dict(folds=1, lambdas=[1.0, 2.0]), dict(fit_intercept=1), dict(pivot="median")):
        with pytest.raises(ValueError):
            ops.ridge(X, y, **bad)
    assert ops.RidgeResult._fields == ("coef", "intercept", "lam", "lambdas", "cv_rmse", "cv_r2", "cv_sse", "path_coef",
                                       "path_intercept", "info", "n_used", "fold_counts")
    res = ops.RidgeResult(*([None] * 12))._replace(coef=torch.tensor([[1.0, 2.0]], dtype=torch.float64),
                                                   intercept=torch.tensor([0.5], dtype=torch.float64))
    assert res.predict(torch.tensor([[1.0, 1.0], [0.0, 2.0]])).tolist() == [[3.5], [4.5]]


def test_lambda_choice_prefers_the_lower_index_among_equals():
    from gae_dgl_amd.ops.ridge import _choose
    nan = float("nan")
    assert _choose([True, True, True], [0.5, 0.25, 0.25]) == 1         # a tie: the lower index
    assert _choose([True, True, True], [0.25, 0.25, 0.25]) == 0
    assert _choose([True, False, True], [0.5, 0.1, 0.4]) == 2           # a lambda whose model failed is never chosen
    assert _choose([False, True, True], [0.1, nan, 0.4]) == 2
    assert _choose([False, False], [0.1, 0.2]) == -1 and _choose([True], [nan]) == -1


BASE = ["--checkpoint", "c.pkl", "--hidden_dims", "32", "16", "--synthetic", "10", "--out", "f.npy"]


@pytest.mark.parametrize("argv, text", [
    (["--ridge"], "--ridge needs --targets"),
    (["--ridge", "0.1", "1"], "--ridge needs --targets"),
    (["--ridge_out", "m.npz"], "need --ridge"),
    (["--ridge_folds", "5"], "need --ridge"),
    (["--targets", "y.npy"], "need --neighbours K"),
    (["--ridge", "--targets", "/no/such/file.npy"], "no such file"),
    (["--ridge", "--targets", "{y}", "--ridge_folds", "1"], "F must lie in 2..32"),
    (["--ridge", "--targets", "{y}", "--ridge_folds", "33"], "F must lie in 2..32"),
    (["--ridge", "-1", "--targets", "{y}"], "finite values >= 0"),
    (["--ridge", "nan", "--targets", "{y}"], "finite values >= 0"),
])
def test_embed_ridge_argument_errors(argv, text, capsys, tmp_path):
    from gae_dgl_amd import embed as E
    np.save(tmp_path / "y.npy", np.zeros(10))
    argv = [a.replace("{y}", str(tmp_path / "y.npy")) for a in argv]
    with pytest.raises(SystemExit):
        E.parse_args(BASE + argv)
    assert text in capsys.readouterr().err


def test_embed_accepts_the_ridge_combinations(tmp_path, capsys):
    from gae_dgl_amd import embed as E
    y = str(tmp_path / "y.npy")
    np.save(y, np.zeros(10))
    a = E.parse_args(BASE + ["--ridge", "--targets", y])
    assert a.ridge == [] and a.ridge_folds is None and a.neighbours is None
    a = E.parse_args(BASE + ["--ridge", "0.01", "1", "100", "--ridge_folds", "3", "--ridge_out", "m.npz", "--targets", y])
    assert a.ridge == [0.01, 1.0, 100.0] and a.ridge_folds == 3 and a.ridge_out == "m.npz"
    a = E.parse_args(BASE + ["--neighbours", "5", "--ridge", "--targets", y])      # both heads on the same targets
    assert a.neighbours == 5 and a.ridge == []
    assert E.parse_args(BASE + ["--neighbours", "5", "--targets", y]).ridge is None
    with pytest.raises(SystemExit):                                    # 3 d = 129 > 128
        E.parse_args(["--checkpoint", "c.pkl", "--hidden_dims", "32", "43", "--synthetic", "10", "--out", "f.npy",
                      "--fused", "off", "--ridge", "--targets", y])
    assert "3 d = 129 must not exceed 128" in capsys.readouterr().err
