"""K28 without a GPU: the numpy restatement tests/logreg_ref.py (its fp64 fixed point against torch's LBFGS on the same
objective; its fp32-pass form on every input the GPU tests fit), the argument errors of the gae_logreg_* entry points
(returned before anything is dereferenced), the workspace query, the option checks of ops.logreg,
metrics.classification_metrics on hand-made tables and the flag parsing of the two command lines."""
import os

import numpy as np
import pytest
import torch

import logreg_ref as R

E_NULL, E_SIZE, E_WORKSPACE, E_RANGE = -1, -2, -5, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the fits of tests/test_gpu_logreg.py: (n, d, c, folds, ragged, lambdas)
FIT_CASES = [(700, 16, 7, 3, False, [0.1, 1.0, 10.0]), (300, 48, 2, 5, True, [0.1, 1.0, 10.0]), (523, 5, 3, 1, False, [1.0])]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    return _lib.load()


def fit_case(n, d, c, F, ragged):
    X, y = R.make_case(n, d, c, seed=n)
    fold = R.deal_folds(n, F, 0, ragged) if F > 1 else np.zeros(n, dtype=np.int64)
    rows = np.concatenate([np.flatnonzero(fold == f) for f in range(F)])
    return X, y, fold, rows, R.pivot_of(X, rows)


def models_of(F, fold, rows):
    """(m, training rows) of every model that has a training set"""
    return [(m, rows if m == F else rows[fold[rows] != m]) for m in range(F + 1) if F > 1 or m == F]


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("n, d, c, lam", [(523, 5, 3, 1.0), (300, 48, 2, 0.1), (700, 16, 7, 10.0)])
def test_the_fp64_reference_reaches_a_stationary_point_not_above_lbfgs(n, d, c, lam):
    X, y, _, rows, p = fit_case(n, d, c, 1, False)
    W, it, conv = R.fit(X, y, rows, lam, c, p, tol=1e-10, max_iter=5000)
    step = R.majoriser_step(X, y, rows, lam, p, W)
    J = R.objective(X, y, rows, lam, p, W)
    # torch.optim.LBFGS in fp64 on the same J, in the same coordinates
    Xa = torch.from_numpy(R.augmented(X, rows, p))
    yt = torch.from_numpy(y[rows])
    Wt = torch.zeros(c, d + 1, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.LBFGS([Wt], max_iter=500, tolerance_grad=1e-12, tolerance_change=1e-14, history_size=20,
                            line_search_fn="strong_wolfe")

    def closure():
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(Xa @ Wt.t(), yt, reduction="sum") + 0.5 * lam * (Wt[:, 1:] ** 2).sum()
        loss.backward()
        return loss
    opt.step(closure)
    J_lbfgs = R.objective(X, y, rows, lam, p, Wt.detach().numpy())
    print(f"{it} passes, majoriser step {step:.3g}, J = {J:.12g}, LBFGS J = {J_lbfgs:.12g}")
    assert conv and step < 1e-9
    assert J <= J_lbfgs * (1 + 1e-12)
    assert np.abs(W.sum(0)).max() < 1e-9                                # the updates sum to zero over the classes


@pytest.mark.parametrize("n, d, c, F, ragged, lams", FIT_CASES)
def test_the_fp32_pass_reference_converges_on_every_input_of_the_gpu_tests(n, d, c, F, ragged, lams):
    X, y, fold, rows, p = fit_case(n, d, c, F, ragged)
    worst = 0
    for lam in lams:
        for m, tr in models_of(F, fold, rows):
            W, it, conv = R.fit(X, y, tr, lam, c, p, tol=1e-5, max_iter=200, dtype=np.float32)
            assert conv, (lam, m, it)
            worst = max(worst, it)
    print(f"at most {worst} passes")
    assert worst <= 200


def test_the_model_maps_through_the_pivot_and_back():
    X, y, _, rows, p = fit_case(120, 4, 3, 1, False)
    W, _, _ = R.fit(X, y, rows, 1.0, 3, p, tol=1e-8)
    coef, icpt = R.to_model(W, p)
    assert np.allclose(R.from_model(coef, icpt, p), W, rtol=0, atol=1e-12)
    Z = X[rows].astype(np.float64) @ coef.T + icpt
    assert np.allclose(Z, R.augmented(X, rows, p) @ W.T, atol=1e-9)
    nll, hit, kept = R.heldout(X, y, rows, coef, icpt)
    assert nll == pytest.approx(R.objective(X, y, rows, 0.0, p, W), rel=1e-12) and hit.shape == kept.shape == (120,)


# ------------------------------------------------------------------ the C ABI's argument errors
def factor_call(lib, *, stats=1 << 20, d=8, c=3, folds=3, lambdas=1 << 21, L=4, n_rows=100, batch=16, coef=1 << 22,
                icpt=1 << 23, info=1 << 24, n_iter=1 << 25, conv=1 << 26, status=1 << 27, ws=1 << 28, ws_bytes=1 << 30):
    rc = lib.gae_logreg_factor(stats, d, c, folds, lambdas, L, n_rows, batch, coef, icpt, info, n_iter, conv, status, ws,
                               ws_bytes, None)
    return rc, lib.gae_last_error().decode()


SHAPE_ERRORS = [
    (dict(d=0), E_RANGE, "d = 0 outside 1..128"),
    (dict(d=129), E_RANGE, "d = 129 outside 1..128"),
    (dict(c=1), E_RANGE, "c = 1 outside 2..32"),
    (dict(c=33), E_RANGE, "c = 33 outside 2..32"),
    (dict(folds=0), E_RANGE, "folds = 0 outside 1..32"),
    (dict(folds=33), E_RANGE, "folds = 33 outside 1..32"),
    (dict(L=0), E_RANGE, "n_lambdas = 0 outside 1..64"),
    (dict(L=65), E_RANGE, "n_lambdas = 65 outside 1..64"),
    (dict(batch=0), E_RANGE, "model_batch = 0 outside 1..16"),
    (dict(batch=17), E_RANGE, "model_batch = 17 outside 1..16"),
    (dict(n_rows=-1), E_SIZE, "negative n_rows = -1"),
    (dict(n_rows=1 << 31), E_SIZE, "beyond int32 row ids"),
    (dict(ws=None), E_NULL, "workspace is NULL"),
    (dict(ws_bytes=16), E_WORKSPACE, "workspace of 16 bytes"),
    (dict(status=None), E_NULL, "status is NULL"),
]


@pytest.mark.parametrize("kw, code, text", SHAPE_ERRORS + [
    (dict(stats=None), E_NULL, "stats / lambdas is NULL"),
    (dict(lambdas=None), E_NULL, "stats / lambdas is NULL"),
    (dict(coef=None), E_NULL, "is NULL"),
    (dict(icpt=None), E_NULL, "is NULL"),
    (dict(info=None), E_NULL, "is NULL"),
    (dict(n_iter=None), E_NULL, "is NULL"),
    (dict(conv=None), E_NULL, "is NULL"),
])
def test_factor_argument_errors_come_before_any_access(lib, kw, code, text):
    rc, msg = factor_call(lib, **kw)
    assert rc == code, (rc, msg)
    assert msg.startswith("gae_logreg_factor: ") and text in msg, msg


def pass_call(lib, *, X=1 << 20, ldx=8, y=1 << 21, n=200, d=8, c=3, pivot=None, rows=1 << 22, n_rows=100, fold_ptr=1 << 23,
              folds=3, L=4, batch=16, lo=0, count=16, flags=0, nll=1 << 24, correct=1 << 25, status=1 << 27, ws=1 << 28,
              ws_bytes=1 << 30):
    rc = lib.gae_logreg_pass(X, ldx, y, n, d, c, pivot, rows, n_rows, fold_ptr, folds, L, batch, lo, count, flags, nll,
                             correct, status, ws, ws_bytes, None)
    return rc, lib.gae_last_error().decode()


@pytest.mark.parametrize("kw, code, text", SHAPE_ERRORS + [
    (dict(lo=-1), E_RANGE, "models -1 .."),
    (dict(count=0), E_RANGE, "outside the 16 models"),
    (dict(lo=8, count=9), E_RANGE, "outside the 16 models"),
    (dict(batch=4, count=5), E_RANGE, "beyond model_batch = 4"),
    (dict(flags=2), E_RANGE, "unknown flags 0x2"),
    (dict(n=-1), E_SIZE, "negative n = -1"),
    (dict(n=1 << 31), E_SIZE, "beyond int32 row ids"),
    (dict(ldx=7), E_SIZE, "ldx 7 < d"),
    (dict(rows=None), E_NULL, "rows / fold_ptr is NULL"),
    (dict(fold_ptr=None), E_NULL, "rows / fold_ptr is NULL"),
    (dict(X=None), E_NULL, "X / y is NULL"),
    (dict(y=None), E_NULL, "X / y is NULL"),
    (dict(flags=1, nll=None), E_NULL, "nll / correct is NULL"),
    (dict(flags=1, correct=None), E_NULL, "nll / correct is NULL"),
])
def test_pass_argument_errors_come_before_any_access(lib, kw, code, text):
    rc, msg = pass_call(lib, **kw)
    assert rc == code, (rc, msg)
    assert msg.startswith("gae_logreg_pass: ") and text in msg, msg


def update_call(lib, *, d=8, c=3, folds=3, lambdas=1 << 21, L=4, n_rows=100, batch=16, lo=0, count=16, it=1, max_iter=10,
                tol=1e-4, pivot=None, coef=1 << 22, icpt=1 << 23, info=1 << 24, n_iter=1 << 25, conv=1 << 26, status=1 << 27,
                ws=1 << 28, ws_bytes=1 << 30):
    rc = lib.gae_logreg_update(d, c, folds, lambdas, L, n_rows, batch, lo, count, it, max_iter, tol, pivot, coef, icpt, info,
                               n_iter, conv, status, ws, ws_bytes, None)
    return rc, lib.gae_last_error().decode()


@pytest.mark.parametrize("kw, code, text", SHAPE_ERRORS + [
    (dict(lo=12, count=5), E_RANGE, "outside the 16 models"),
    (dict(it=0), E_RANGE, "iteration = 0 outside 1..max_iter = 10"),
    (dict(it=11), E_RANGE, "iteration = 11 outside 1..max_iter = 10"),
    (dict(tol=-1.0), E_RANGE, "tol = -1 is negative or not finite"),
    (dict(tol=float("nan")), E_RANGE, "is negative or not finite"),
    (dict(lambdas=None), E_NULL, "lambdas is NULL"),
    (dict(coef=None), E_NULL, "is NULL"),
    (dict(n_iter=None), E_NULL, "is NULL"),
])
def test_update_argument_errors_come_before_any_access(lib, kw, code, text):
    rc, msg = update_call(lib, **kw)
    assert rc == code, (rc, msg)
    assert msg.startswith("gae_logreg_update: ") and text in msg, msg


def predict_call(lib, *, X=1 << 20, ldx=8, n=100, d=8, c=3, coef=1 << 21, icpt=1 << 22, pivot=None, labels=1 << 23,
                 proba=1 << 24, ldp=3, status=1 << 25):
    rc = lib.gae_logreg_predict(X, ldx, n, d, c, coef, icpt, pivot, labels, proba, ldp, status, None)
    return rc, lib.gae_last_error().decode()


@pytest.mark.parametrize("kw, code, text", [
    (dict(d=0), E_RANGE, "d = 0 outside 1..128"),
    (dict(d=129, ldx=129), E_RANGE, "d = 129 outside 1..128"),
    (dict(c=1), E_RANGE, "c = 1 outside 2..32"),
    (dict(c=33, ldp=33), E_RANGE, "c = 33 outside 2..32"),
    (dict(n=-1), E_SIZE, "negative n = -1"),
    (dict(n=1 << 31), E_SIZE, "beyond int32 row ids"),
    (dict(ldx=7), E_SIZE, "ldx 7 < d"),
    (dict(ldp=2), E_SIZE, "ldp 2 < c"),
    (dict(coef=None), E_NULL, "coef / intercept is NULL"),
    (dict(icpt=None), E_NULL, "coef / intercept is NULL"),
    (dict(X=None), E_NULL, "X / labels is NULL"),
    (dict(labels=None), E_NULL, "X / labels is NULL"),
    (dict(status=None), E_NULL, "status is NULL"),
])
def test_predict_argument_errors_come_before_any_access(lib, kw, code, text):
    rc, msg = predict_call(lib, **kw)
    assert rc == code, (rc, msg)
    assert msg.startswith("gae_logreg_predict: ") and text in msg, msg
    assert predict_call(lib, proba=None, ldp=0, n=0)[0] == 0           # no rows: nothing to launch, no GPU needed


def expected_bytes(n_rows, d, c, F, L, batch):
    """the layout of csrc/logreg.hip: every region rounded up to 256 bytes"""
    from gae_dgl_amd import ops
    up = lambda v: (v + 255) // 256 * 256
    M, D1 = (F + 1) * L, d + 1
    slabs = -(-(-(-n_rows // ops.LOGREG_CHUNK_ROWS) + F) // ops.LOGREG_SLAB_CHUNKS)
    return (up(M * D1 * (D1 + 1) // 2 * 8) + 2 * up(M * c * D1 * 8) + up(M * 8) + up(M * c * D1 * 4) + 2 * up(M * 4)
            + up(slabs * batch * c * D1 * 4) + 2 * up(slabs * batch * 8))


def test_workspace_query_is_a_monotone_host_function(lib):
    q = lib.gae_logreg_workspace_bytes
    from gae_dgl_amd import ops
    C = ops.LOGREG_CHUNK_ROWS * ops.LOGREG_SLAB_CHUNKS
    assert (ops.LOGREG_CHUNK_ROWS, ops.LOGREG_SLAB_CHUNKS) == (64, 8)
    assert q(0, 1, 2, 1, 1, 1) > 0 and q(1000, 48, 2, 5, 13, 78) == q(1000, 48, 2, 5, 13, 78)
    for d, c, F, L in ((1, 2, 1, 1), (48, 2, 5, 13), (128, 32, 32, 64)):
        M = (F + 1) * L
        prev = 0
        for n in (0, 1, C - 1, C, C + 1, 2 * C + 3, 19717, 249455, 10 ** 6, 2 ** 31 - 1):
            cur = q(n, d, c, F, L, 1)
            assert cur >= prev > -1, (n, d, c, F, L)
            prev = cur
        prev = 0
        for batch in sorted({1, 2, M // 2 + 1, M}):                    # ... in the models of a launch
            cur = q(19717, d, c, F, L, batch)
            assert cur >= prev > -1
            prev = cur
    prev = 0
    for F, L in ((1, 1), (1, 2), (2, 2), (5, 13), (32, 64)):            # ... and in the model count
        cur = q(19717, 16, 3, F, L, 1)
        assert cur >= prev > -1
        prev = cur
    # pinned at three shapes
    for shape, nbytes in (((1128, 48, 2, 5, 13, 78), 1015296), ((19717, 16, 3, 5, 13, 78), 864256),
                          ((249455, 48, 2, 5, 13, 26), 6096384)):
        assert q(*shape) == expected_bytes(*shape) == nbytes, shape
    assert q(10, 0, 2, 1, 1, 1) == E_RANGE and q(10, 129, 2, 1, 1, 1) == E_RANGE and q(10, 8, 1, 1, 1, 1) == E_RANGE
    assert q(10, 8, 33, 1, 1, 1) == E_RANGE and q(10, 8, 2, 33, 1, 1) == E_RANGE and b"folds = 33" in lib.gae_last_error()
    assert q(10, 8, 2, 1, 65, 1) == E_RANGE and q(10, 8, 2, 1, 1, 3) == E_RANGE
    assert q(-1, 8, 2, 1, 1, 1) == E_SIZE and q(1 << 31, 8, 2, 1, 1, 1) == E_SIZE


def test_the_constants_are_the_headers():
    import re
    from gae_dgl_amd import ops, _lib
    text = open(os.path.join(ROOT, "include", "gae_hip_experimental.h")).read()
    assert int(re.search(r"GAE_LOGREG_CHUNK_ROWS = (\d+)", text).group(1)) == ops.LOGREG_CHUNK_ROWS == _lib.LOGREG_CHUNK_ROWS
    assert int(re.search(r"GAE_LOGREG_SLAB_CHUNKS = (\d+)", text).group(1)) == ops.LOGREG_SLAB_CHUNKS
    assert (ops.LOGREG_MAX_D, ops.LOGREG_MAX_CLASSES, ops.LOGREG_MAX_FOLDS, ops.LOGREG_MAX_LAMBDAS) == (128, 32, 32, 64)
    for name in ("gae_logreg_workspace_bytes", "gae_logreg_factor", "gae_logreg_pass", "gae_logreg_update",
                 "gae_logreg_predict"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\(" % name, text)


# ------------------------------------------------------------------ the wrapper
def test_ops_logreg_has_no_cpu_fallback_and_checks_its_options():
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    g = torch.Generator().manual_seed(0)
    X, y = torch.randn(60, 4, generator=g), torch.arange(60) % 3
    with pytest.raises(GaeHipError):
        ops.logreg(X, y)                                               # CPU tensors
    with pytest.raises(GaeHipError):
        ops.logreg_predict(X, torch.zeros(3, 4), torch.zeros(3))
    empty = torch.arange(60) % 4
    empty[empty == 2] = -1                                             # fold 2 holds no rows
    for bad in (dict(y=torch.zeros(60, dtype=torch.int64)),            # c = 1
                dict(n_classes=1), dict(n_classes=33), dict(y=torch.arange(60) % 33), dict(n_classes=2),
                dict(X=torch.randn(60, 129)), dict(X=torch.randn(60, 0)), dict(y=y.float()), dict(y=y[:50]),
                dict(y=y - 2), dict(lambdas=[-1.0]), dict(lambdas=[float("nan")]), dict(lambdas=[]), dict(lambdas=[1.0] * 65),
                dict(folds=0), dict(folds=33), dict(folds=2.5), dict(folds=True), dict(folds=1, lambdas=[1.0, 2.0]),
                dict(folds=4, fold=empty), dict(folds=3, fold=torch.arange(60) % 4), dict(folds=3, fold=empty.float()),
                dict(max_iter=0), dict(check_every=0), dict(tol=-1.0), dict(tol=float("inf")), dict(model_batch=0)):
        kw = dict(bad)
        with pytest.raises(ValueError):
            ops.logreg(kw.pop("X", X), kw.pop("y", y), **kw)
    assert ops.LogRegResult._fields[:18] == (
        "coef", "intercept", "lam", "lambdas", "cv_logloss", "cv_accuracy", "cv_nll", "cv_correct", "path_coef",
        "path_intercept", "info", "n_iter", "converged", "train_logloss", "n_used", "fold_counts", "class_counts", "pivot")
    res = ops.LogRegResult(*([None] * len(ops.LogRegResult._fields)))._replace(
        coef=torch.tensor([[1.0, 2.0], [0.0, -1.0]], dtype=torch.float64), intercept=torch.tensor([0.5, -0.5], dtype=torch.float64))
    lin = res.to_torch()
    assert isinstance(lin, torch.nn.Linear) and lin.weight.dtype == torch.float32
    assert lin(torch.tensor([[1.0, 1.0]])).tolist() == [[3.5, -1.5]]


def test_the_models_carry_the_classification_methods():
    import gae_dgl_amd as G
    from gae_dgl_amd.vgae import VGAE
    assert callable(G.GAE.classify_nodes) and callable(VGAE.classify_nodes) and callable(G.GAE.logreg_graphs)
    assert VGAE.classify_nodes is not G.GAE.classify_nodes             # on mu, not on a tuple


# ------------------------------------------------------------------ metrics
def test_classification_metrics_on_hand_made_tables():
    from gae_dgl_amd import metrics
    true = torch.tensor([0, 0, 0, 1, 1, 2, 2, 2, 2, -1])
    pred = torch.tensor([0, 0, 1, 1, 2, 2, 2, 2, 0, 1])
    m = metrics.classification_metrics(pred, true)
    assert m["confusion"] == [[2, 1, 0], [0, 1, 1], [1, 0, 3]] and m["n"] == 9 and m["unpredicted"] == 0
    assert m["accuracy"] == pytest.approx(6 / 9)
    assert m["precision"] == pytest.approx([2 / 3, 1 / 2, 3 / 4]) and m["recall"] == pytest.approx([2 / 3, 1 / 2, 3 / 4])
    assert m["macro_f1"] == pytest.approx((2 / 3 + 1 / 2 + 3 / 4) / 3)
    assert "log_loss" not in m and "roc_auc" not in m
    # two classes with probabilities: log-loss by hand, the AUC through roc_auc; a class nobody is called
    true = torch.tensor([1, 0, 1, 0, -1])
    proba = torch.tensor([[0.2, 0.8], [0.6, 0.4], [0.7, 0.3], [0.9, 0.1], [0.5, 0.5]])
    pred = proba.argmax(1)
    m = metrics.classification_metrics(pred, true, proba)
    assert m["confusion"] == [[2, 0], [1, 1]] and m["accuracy"] == 0.75
    assert m["log_loss"] == pytest.approx(-(np.log(0.8) + np.log(0.6) + np.log(0.3) + np.log(0.9)) / 4)
    assert m["roc_auc"] == pytest.approx(metrics.roc_auc(torch.tensor([0.8, 0.3]), torch.tensor([0.4, 0.1]))) == 0.75
    m = metrics.classification_metrics(torch.tensor([0, 0]), torch.tensor([0, 1]), n_classes=3)
    assert m["confusion"] == [[1, 0, 0], [1, 0, 0], [0, 0, 0]] and m["precision"] == [0.5, 0.0, 0.0]
    assert m["recall"] == [1.0, 0.0, 0.0] and m["macro_f1"] == pytest.approx((2 / 3 + 0.0) / 2)
    # a row without a prediction is an error, is in no column and is counted
    m = metrics.classification_metrics(torch.tensor([-1, 1]), torch.tensor([1, 1]),
                                       torch.tensor([[float("nan")] * 2, [0.25, 0.75]]))
    assert m["accuracy"] == 0.5 and m["unpredicted"] == 1 and m["confusion"] == [[0, 0], [0, 1]]
    assert m["log_loss"] == pytest.approx(-np.log(0.75)) and np.isnan(m["roc_auc"])
    with pytest.raises(ValueError):
        metrics.classification_metrics(torch.tensor([0, 1]), torch.tensor([0]))
    with pytest.raises(ValueError):
        metrics.classification_metrics(torch.tensor([0, 3]), torch.tensor([0, 1]), n_classes=3)
    with pytest.raises(ValueError):
        metrics.classification_metrics(torch.tensor([0, 1]), torch.tensor([0, 1]), torch.zeros(2, 3), n_classes=2)


# ------------------------------------------------------------------ the command lines
BASE = ["--checkpoint", "c.pkl", "--hidden_dims", "32", "16", "--synthetic", "10", "--out", "f.npy"]


@pytest.mark.parametrize("argv, text", [
    (["--logreg"], "--logreg needs --labels"),
    (["--logreg", "0.1", "1"], "--logreg needs --labels"),
    (["--logreg_out", "m.npz"], "need --logreg"),
    (["--logreg_folds", "5"], "need --logreg"),
    (["--labels", "{y}"], "need --logreg"),
    (["--logreg", "--labels", "/no/such/file.npy"], "no such file"),
    (["--logreg", "--labels", "{y}", "--logreg_folds", "1"], "F must lie in 2..32"),
    (["--logreg", "--labels", "{y}", "--logreg_folds", "33"], "F must lie in 2..32"),
    (["--logreg", "-1", "--labels", "{y}"], "finite values >= 0"),
    (["--logreg", "nan", "--labels", "{y}"], "finite values >= 0"),
])
def test_embed_logreg_argument_errors(argv, text, capsys, tmp_path):
    from gae_dgl_amd import embed as E
    np.save(tmp_path / "y.npy", np.zeros(10, dtype=np.int64))
    argv = [a.replace("{y}", str(tmp_path / "y.npy")) for a in argv]
    with pytest.raises(SystemExit):
        E.parse_args(BASE + argv)
    assert text in capsys.readouterr().err


def test_embed_accepts_the_logreg_combinations(tmp_path, capsys):
    from gae_dgl_amd import embed as E
    y = str(tmp_path / "y.npy")
    np.save(y, np.zeros(10, dtype=np.int64))
    a = E.parse_args(BASE + ["--logreg", "--labels", y])
    assert a.logreg == [] and a.logreg_folds is None and a.ridge is None
    a = E.parse_args(BASE + ["--logreg", "0.01", "1", "100", "--logreg_folds", "3", "--logreg_out", "m.npz", "--labels", y])
    assert a.logreg == [0.01, 1.0, 100.0] and a.logreg_folds == 3 and a.logreg_out == "m.npz"
    a = E.parse_args(BASE + ["--logreg", "--labels", y, "--ridge", "--forest", "--mlp", "--neighbours", "5", "--targets", y])
    assert a.logreg == [] and a.ridge == [] and a.forest == 100 and a.mlp == [] and a.neighbours == 5
    assert E.parse_args(BASE).logreg is None
    with pytest.raises(SystemExit):                                    # 3 d = 129 > 128
        E.parse_args(["--checkpoint", "c.pkl", "--hidden_dims", "32", "43", "--synthetic", "10", "--out", "f.npy",
                      "--fused", "off", "--logreg", "--labels", y])
    assert "3 d = 129 must not exceed 128" in capsys.readouterr().err


@pytest.mark.parametrize("argv, text", [
    (["--classify_folds", "5"], "need --classify"),
    (["--classify_out", "m.npz"], "need --classify"),
    (["--classify_seed", "1"], "need --classify"),
    (["--classify_test_frac", "0.3"], "need --classify"),
    (["--classify", "--classify_folds", "1"], "F must lie in 2..32"),
    (["--classify", "--classify_folds", "33"], "F must lie in 2..32"),
    (["--classify", "--classify_test_frac", "0"], "Q must lie inside (0, 1)"),
    (["--classify", "--classify_test_frac", "1"], "Q must lie inside (0, 1)"),
    (["--classify", "-1"], "finite values >= 0"),
    (["--classify", "inf"], "finite values >= 0"),
])
def test_train_transductive_classify_argument_errors(argv, text, capsys):
    from gae_dgl_amd import train_transductive as TT
    with pytest.raises(SystemExit):
        TT.parse_args(argv)
    assert text in capsys.readouterr().err


def test_train_transductive_accepts_the_classify_flags():
    from gae_dgl_amd import train_transductive as TT
    a = TT.parse_args(["--classify"])
    assert a.classify == [] and a.classify_folds is None and a.classify_test_frac is None and a.classify_out is None
    a = TT.parse_args(["--classify", "0.1", "10", "--classify_folds", "3", "--classify_test_frac", "0.25", "--classify_seed", "4",
                       "--classify_out", "m.npz", "--knn", "5", "--cluster", "3"])
    assert a.classify == [0.1, 10.0] and a.classify_folds == 3 and a.classify_test_frac == 0.25 and a.classify_seed == 4
    assert a.classify_out == "m.npz" and a.knn == 5 and a.cluster == 3
    assert TT.parse_args([]).classify is None
