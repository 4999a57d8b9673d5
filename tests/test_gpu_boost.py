"""K30 on the device (ops.boost, ops.boost_predict, GAE.boost_graphs, embed --boost) against tests/boost_ref.py: every
returned field bit for bit (only the "logistic" cv_curve, which goes through the library's log1p, at rel 1e-12)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boost_ref as B  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = ["feature", "threshold_bin", "threshold", "left", "count", "value", "gain", "n_nodes", "edges", "n_edges",
          "importances", "info", "train_score"]
SCALARS = ["base_score", "lr", "lam", "best_round", "best_cfg", "cv_rmse", "cv_r2", "cv_accuracy", "objective", "n_used"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(v):
    return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def _same(a, b, what):
    """ints equal, floats by bit pattern, NaN in the same places"""
    a, b = _np(a), _np(b)
    assert a.shape == b.shape, f"{what}: shape {a.shape} vs {b.shape}"
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        assert a.dtype == b.dtype, f"{what}: {a.dtype} vs {b.dtype}"
        na, nb = np.isnan(a), np.isnan(b)
        assert np.array_equal(na, nb), f"{what}: NaN in other places"
        ints = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
        ia, ib = np.where(na, 0, a).view(ints), np.where(nb, 0, b).view(ints)
        assert np.array_equal(ia, ib), f"{what}: {int((ia != ib).sum())} of {a.size} values differ in bits, max |diff| " \
                                       f"{np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64)))}"
    else:
        assert np.array_equal(a, b), f"{what}: {int((a != b).sum())} of {a.size} values differ"


def _same_scalar(a, b, what):
    if isinstance(a, float) or isinstance(b, float):
        _same(np.float64(a), np.float64(b), what)
    else:
        assert a == b, f"{what}: {a!r} vs {b!r}"


def _fit(X, y, objective, R, **kw):
    import gae_dgl_amd.ops as ops
    kw = dict(kw)
    for name in ("fold", "rows"):
        if isinstance(kw.get(name), np.ndarray):
            kw[name] = _dev(kw[name])
    return ops.boost(X if isinstance(X, torch.Tensor) else _dev(X), _dev(y), objective, R, **kw)


def _against_ref(res, ref):
    for name in TABLES:
        _same(getattr(res, name), getattr(ref, name), name)
    for name in SCALARS:
        _same_scalar(getattr(res, name), getattr(ref, name), name)
    if ref.objective == "logistic":
        np.testing.assert_allclose(_np(res.cv_curve), ref.cv_curve, rtol=1e-12, atol=0, err_msg="cv_curve")
        np.testing.assert_allclose(res.cv_logloss, ref.cv_logloss, rtol=1e-12, atol=0, err_msg="cv_logloss")
    else:
        _same(res.cv_curve, ref.cv_curve, "cv_curve")
        _same_scalar(res.cv_logloss, ref.cv_logloss, "cv_logloss")


def _regression(n, d, seed, noise=0.1):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)).astype(np.float32)
    y = (X[:, 0] * X[:, min(1, d - 1)] + np.sin(2 * X[:, d - 1]) + noise * rng.normal(size=n)).astype(np.float32)
    return X, y


def _xor(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, 2)).astype(np.float32)
    return X, (X[:, 0] * X[:, 1] > 0).astype(np.int64)


def _case(name):
    """(X, y, objective, n_rounds, keywords): the smallest shapes at which each path can break"""
    if name == "small":
        X, y = _regression(300, 5, 0)
        return X, y, "squared", 6, dict(max_depth=3, max_bins=8)
    if name == "two_tiles":                                            # 256 bins x 20 bytes: 12 features per tile
        X, y = _regression(400, 14, 1)
        return X, y, "squared", 3, dict(max_depth=3, max_bins=256, folds=2)
    if name == "root_across_blocks":                                   # the all-rows model's root: two chunks
        X, y = _regression(B.SPLIT_ROWS + 5, 3, 2)
        return X, y, "squared", 3, dict(max_depth=2, folds=2, max_bins=16)
    if name == "long_children_tiles":                                  # long nodes below the root, their slots in two tiles
        X, y = _regression(3 * B.SPLIT_ROWS + 7, 13, 12)
        return X, y, "squared", 2, dict(max_depth=3, folds=2, max_bins=256)
    if name == "depth8":
        X, y = _regression(200, 4, 3)
        return X, y, "squared", 3, dict(max_depth=8, folds=2, learning_rates=(0.5,), lambdas=(0.0,))
    if name == "min_samples_leaf":
        X, y = _regression(300, 5, 4)
        return X, y, "squared", 4, dict(max_depth=4, min_samples_leaf=7, folds=3)
    if name == "max_features":
        X, y = _regression(300, 10, 5)
        return X, y, "squared", 4, dict(max_depth=3, max_features=3, folds=3, seed=11)
    if name == "duplicated_rows":
        X, y = _regression(60, 4, 6)
        X, y = np.tile(X, (5, 1)), np.tile(y, 5)
        return X, y, "squared", 4, dict(max_depth=4, folds=3)
    if name == "two_bins":
        X, y = _regression(300, 5, 7)
        return X, y, "squared", 4, dict(max_depth=3, max_bins=2, folds=3)
    if name == "grid":
        X, y = _regression(300, 5, 8)
        return X, y, "squared", 8, dict(max_depth=2, learning_rates=(0.5, 0.1), lambdas=(0.0, 4.0), folds=3)
    if name == "fold_minus_one":
        X, y = _regression(330, 5, 9)
        fold = (np.arange(330) % 4 - 1).astype(np.int64)               # a quarter of the rows is a test set
        return X, y, "squared", 4, dict(max_depth=3, folds=3, fold=fold)
    if name == "logistic_small":
        X, y = _xor(300, 10)
        y[::17] = -1
        return X, y, "logistic", 8, dict(max_depth=3, learning_rates=(0.3,), folds=3, max_bins=16)
    if name == "logistic_separable":                                   # scores saturate, H cells reach 0, the splits stop
        X = np.c_[np.linspace(-1, 1, 64), np.tile([0.0, 1.0], 32)].astype(np.float32)
        y = (X[:, 0] > 0).astype(np.int64)
        return X, y, "logistic", 40, dict(max_depth=1, learning_rates=(1.0,), lambdas=(0.0,), min_child_weight=1e-9, folds=2,
                                          seed=1)
    raise KeyError(name)


CASES = ["small", "two_tiles", "root_across_blocks", "long_children_tiles", "depth8", "min_samples_leaf", "max_features", "duplicated_rows", "two_bins",
         "grid", "fold_minus_one", "logistic_small", "logistic_separable"]


@pytest.mark.parametrize("name", CASES)
def test_bit_for_bit_against_the_reference(name):
    X, y, objective, R, kw = _case(name)
    ref = B.boost(X, y, objective, R, **kw)
    res = _fit(X, y, objective, R, **kw)
    _against_ref(res, ref)
    if name == "logistic_separable":                                   # the case is what it says
        assert int(ref.n_nodes[0]) == 3 and int(ref.n_nodes[-1]) == 1 and float(ref.value[-1, 0]) == 0.0
    if name == "depth8":
        k = int(ref.n_nodes[0])
        assert int(ref.count[0, :k][ref.feature[0, :k] < 0].min()) == 1 and k > 2 ** 5
    if name == "root_across_blocks":
        assert int(ref.count[0, 0]) == B.SPLIT_ROWS + 5
    if name == "long_children_tiles":                                  # the all-rows model's first tree
        assert int(ref.count[0, 1]) > B.SPLIT_ROWS and int(ref.count[0, 2]) > B.SPLIT_ROWS and X.shape[1] > 12


@pytest.fixture(scope="module")
def base():
    X, y = _regression(500, 6, 20)
    kw = dict(max_depth=3, learning_rates=(0.3, 0.1), lambdas=(1.0,), folds=3, max_bins=32)
    return X, y, kw, _fit(X, y, "squared", 18, **kw)


def _equal_results(a, b, skip=()):
    for name in TABLES + ["cv_curve"]:
        if name not in skip:
            _same(getattr(a, name), getattr(b, name), name)
    for name in SCALARS + ["cv_logloss"]:
        if name not in skip:
            _same_scalar(getattr(a, name), getattr(b, name), name)


def test_same_bits_across_runs_streams_strides_rows_and_checks(base):
    X, y, kw, first = base
    _equal_results(first, _fit(X, y, "squared", 18, **kw))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _fit(X, y, "squared", 18, **kw)
    side.synchronize()
    _equal_results(first, other)
    wide = torch.full((500, 11), float("nan"), device="cuda")
    wide[:, 2:8] = _dev(X)
    _equal_results(first, _fit(wide[:, 2:8], y, "squared", 18, **kw))
    _equal_results(first, _fit(X, y, "squared", 18, check_every=1, **kw))
    mask = np.arange(500) % 3 != 1
    by_mask = _fit(X, y, "squared", 18, rows=mask, **kw)
    by_ids = _fit(X, y, "squared", 18, rows=np.nonzero(mask)[0][::-1].copy(), **kw)
    _equal_results(by_mask, by_ids)


def test_a_configuration_alone_gives_the_bits_it_gives_inside_the_grid(base):
    X, y, kw, grid = base
    alone = _fit(X, y, "squared", 18, **dict(kw, learning_rates=(grid.lr,), lambdas=(grid.lam,)))
    _equal_results(grid, alone, skip=("cv_curve", "info", "best_cfg"))
    _same(grid.cv_curve[grid.best_cfg], alone.cv_curve[0], "cv_curve of the chosen configuration")


def test_prediction(base):
    X, y, kw, res = base
    ref = B.boost(X, y, "squared", 18, **kw)
    rng = np.random.default_rng(21)
    Xt = rng.normal(size=(77, 6)).astype(np.float32)
    _same(res.predict(_dev(Xt)), B.predict(ref, Xt), "predict")
    _same(res.predict(_dev(X), n_rounds=18), res.train_score, "predict(X_train) vs train_score")
    for r in (0, 1, 7):
        _same(res.predict(_dev(Xt), n_rounds=r), B.predict(ref, Xt, n_rounds=r), f"the prefix model of {r} rounds")
    # a row exactly on the root's threshold goes left, the next float up goes right
    f, thr, left = int(ref.feature[0, 0]), ref.threshold[0, 0], int(ref.left[0, 0])
    assert f >= 0
    on = np.zeros((2, 6), np.float32)
    on[:, f] = [thr, np.nextafter(thr, np.float32(np.inf))]
    got = _np(res.predict(_dev(on), n_rounds=1))
    for i, node in enumerate((left, left + 1)):                        # the rest of the walk from the child the rule names
        while ref.feature[0, node] >= 0:
            node = ref.left[0, node] + (0 if on[i, ref.feature[0, node]] <= ref.threshold[0, node] else 1)
        assert got[i] == ref.base_score + ref.value[0, node]
    # a NaN feature: a NaN row and a status count
    Xt[5, 2] = np.nan
    Xt[9, 0] = np.inf
    status = torch.zeros(4, dtype=torch.int64, device="cuda")
    import gae_dgl_amd.ops as ops
    out = _np(ops.boost_predict(res, _dev(Xt), status=status))
    assert np.isnan(out[[5, 9]]).all() and np.isfinite(np.delete(out, [5, 9])).all()
    assert status.tolist()[:2] == [2, 0]


def test_rows_and_errors():
    from gae_dgl_amd._lib import GaeHipError
    X, y = _regression(300, 5, 30)
    fold = B.default_fold(300, 3, 0)
    fold[::7] = -1
    rows = np.arange(300) % 5 != 0
    kw = dict(max_depth=3, folds=3)
    clean = _fit(X, y, "squared", 5, fold=fold, rows=rows, **kw)
    Xp, yp = X.copy(), y.copy()
    out = ~rows | (fold < 0)
    Xp[out] = np.nan
    yp[out] = np.inf
    _equal_results(clean, _fit(Xp, yp, "squared", 5, fold=fold, rows=rows, **kw))
    Xb = X.copy()
    Xb[np.nonzero(~out)[0][3], 1] = np.inf
    with pytest.raises(GaeHipError):
        _fit(Xb, y, "squared", 5, fold=fold, rows=rows, **kw)
    yb = y.copy()
    yb[np.nonzero(~out)[0][5]] = np.nan
    with pytest.raises(GaeHipError):
        _fit(X, yb, "squared", 5, fold=fold, rows=rows, **kw)
    # label -1 rows are never read
    Xl, yl = _xor(300, 31)
    yl[::9] = -1
    lkw = dict(max_depth=2, folds=3, learning_rates=(0.3,))
    clean = _fit(Xl, yl, "logistic", 5, **lkw)
    Xq = Xl.copy()
    Xq[yl < 0] = np.nan
    _equal_results(clean, _fit(Xq, yl, "logistic", 5, **lkw))
    with pytest.raises(GaeHipError):
        _fit(Xl, np.where(yl < 0, 2, yl), "logistic", 5, **lkw)


def test_the_selection_rule_on_the_returned_curve():
    X, y = _regression(300, 5, 40, noise=1.0)
    res = _fit(X, y, "squared", 25, max_depth=3, learning_rates=(1.0, 0.5, 0.1), lambdas=(0.0, 1.0), folds=3)
    curve = _np(res.cv_curve)
    assert curve.shape == (6, 25) and _np(res.info).tolist() == [0] * 6
    best = (0, 0)
    for c in range(6):
        for r in range(25):
            if curve[c, r] < curve[best]:
                best = (c, r)
    assert (res.best_cfg, res.best_round) == (best[0], best[1] + 1)
    assert (res.lr, res.lam) == [(a, b) for a in (1.0, 0.5, 0.1) for b in (0.0, 1.0)][best[0]]
    assert res.cv_rmse == math.sqrt(curve[best])


def test_xor_is_learnt_where_a_linear_model_is_not():
    import gae_dgl_amd.ops as ops
    X, y = _xor(600, 0)
    fold = B.default_fold(600, 5, 0)
    res = _fit(X, y, "logistic", 20, max_depth=2, learning_rates=(0.3,), max_bins=32, folds=5, fold=fold)
    lin = ops.logreg(_dev(X), _dev(y), [1.0], folds=5, fold=_dev(fold))
    print(f"boost held-out accuracy {res.cv_accuracy:.4f}, logreg {float(lin.cv_accuracy[0]):.4f}")
    assert res.cv_accuracy >= 0.9
    assert float(lin.cv_accuracy[0]) <= 0.65
    proba = _np(res.predict_proba(_dev(X)))
    assert ((proba >= 0.5) == (y == 1)).mean() >= 0.9


def test_boost_graphs_is_boost_of_the_molecule_features():
    import gae_dgl_amd as G
    from gae_dgl_amd import ops
    from gae_dgl_amd.dataset import DeviceGraphDataset
    dev = torch.device("cuda")
    data = DeviceGraphDataset.synthetic_zinc(300, seed=1, device=dev)
    torch.manual_seed(0)
    model = G.GAE(39, [32, 16]).to(dev).eval()
    feats = model.embed_graphs(data)
    y = (feats[:, 0] * 3 + feats[:, 17]).float().contiguous()
    kw = dict(max_depth=3, learning_rates=(0.3,), folds=3, seed=3)
    want = ops.boost(feats, y, "squared", 6, **kw)
    _equal_results(model.boost_graphs(data, y, "squared", 6, fused="auto", batch_size=128, **kw), want)
    assert want.feature.shape == (6, 15) and want.edges.shape[0] == 48 and want.n_used == 300
    labels = (y > y.median()).long()
    _equal_results(model.boost_graphs(data, labels, "logistic", 4, **kw), ops.boost(feats, labels, "logistic", 4, **kw))
    with pytest.raises(ValueError):
        model.boost_graphs(data, y, grad=True)


def test_cli_embed_boost_in_a_fresh_process(tmp_path):
    import gae_dgl_amd as G
    torch.manual_seed(0)
    ckpt = str(tmp_path / "m.pkl")
    torch.save(G.GAE(39, [32, 16]).state_dict(), ckpt)
    ng = 300
    rng = np.random.default_rng(1)
    labels = rng.integers(0, 2, ng)
    labels[:7] = -1
    np.save(tmp_path / "labels.npy", labels)
    np.save(tmp_path / "y.npy", rng.normal(size=ng).astype(np.float32))
    run = subprocess.run([sys.executable, "-m", "gae_dgl_amd.embed", "--checkpoint", ckpt, "--hidden_dims", "32", "16",
                          "--synthetic", str(ng), "--out", str(tmp_path / "f.npy"), "--boost", "12", "--boost_depth", "2",
                          "--boost_lr", "0.3", "0.1", "--boost_lambda", "1", "--boost_folds", "3", "--boost_out",
                          str(tmp_path / "model.npz"), "--targets", str(tmp_path / "y.npy"), "--labels",
                          str(tmp_path / "labels.npy")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = [l for l in run.stdout.splitlines() if l.startswith("Boosting (")]
    assert len(lines) == 2, run.stdout
    assert " of 12 rounds, depth 2, 3-fold CV, lr = " in lines[0] and ", lambda = 1) RMSE: " in lines[0] and " | R2: " in lines[0]
    assert " of 12 rounds, depth 2, 3-fold CV, lr = " in lines[1] and ") accuracy: " in lines[1] \
        and " | ROC-AUC: " in lines[1] and " | log-loss: " in lines[1]
    assert f"Boosted squared trees on {ng} molecules, 8 models side by side" in run.stdout
    assert f"Boosted logistic trees on {ng - 7} molecules, 8 models side by side" in run.stdout
    z = np.load(tmp_path / "model.npz")
    assert z["feature"].shape == (12, 7) and z["value"].dtype == np.float64 and z["edges"].shape[0] == 48
    assert 1 <= int(z["best_round"]) <= 12 and float(z["lr"]) in (0.3, 0.1) and z["cv_curve"].shape == (2, 12)
