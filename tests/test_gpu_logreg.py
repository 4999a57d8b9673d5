"""K28 on the device (gae_logreg_*, ops.logreg / logreg_predict, GAE.classify_nodes, GAE.logreg_graphs, the two scripts)
against tests/logreg_ref.py.  What is compared and why:

1. the first pass: from W = 0 every probability is 1 / c, so after ``max_iter=1`` W = -A^-1 X~^T (1 / c - Y); compared
   with the fp64 reference.  FIRST_TOL is 4 x the deviation measured on an MI355X, max |W - W64| / max |W64| per shape
   (measured: 5.99e-7, 5.66e-7, 5.90e-7, 7.16e-7, with folds 1.71e-6, strided 5.66e-7; the fp32-numpy reference's own
   deviation on the same inputs: 6.74e-7, 1.12e-6, 5.90e-7, 5.77e-7, 1.72e-6, 1.12e-6 -- the device is within 1.3 x of it);
2. a converged fit: for the device's (b, W) of EVERY model the host checks in fp64 that the majoriser step of the exact
   gradient is <= 2 tol max(1, max|W|), that J is above the reference optimum (tol = 1e-10) by at most 1e-5 relative and
   that the parameters sum to 0 over the classes to 1e-4.  Coefficients are not compared entry by entry: J is flat;
3. the CV tables recomputed in fp64 at the device's own coefficients; the choice of lambda from the returned table;
4. rows that are not listed are never read; the same bits for any stride, check_every, model_batch, company and stream;
5. a list long enough for the 64-lane order of the slab partials; predict; errors; the model methods and the scripts."""
import functools
import os

import numpy as np
import pytest
import torch

import logreg_ref as R

pytestmark = pytest.mark.gpu
C = 64                                                                  # GAE_LOGREG_CHUNK_ROWS
TOL = 1e-5
# (n, d, c, folds, pad): 4 x the measured deviation (the docstring)
FIRST_TOL = {(523, 5, 3, 1, 0): 4 * 5.99e-7, (700, 16, 7, 1, 0): 4 * 5.66e-7, (300, 48, 2, 1, 0): 4 * 5.90e-7,
             (600, 128, 32, 1, 0): 4 * 7.16e-7, (3 * (2 * C + 1), 16, 7, 3, 0): 4 * 1.71e-6, (700, 16, 7, 1, 8): 4 * 5.66e-7}
ROW_TOL = {(700, 16, 7): 4 * 5.66e-7, (300, 48, 2): 4 * 5.90e-7}        # per held-out row, for cv_nll
PROBA_TOL = 4 * 1.2e-6                                                  # measured on the predict test's 831 rows: 1.20e-6
FIT_CASES = [(700, 16, 7, 3, False, (0.1, 1.0, 10.0)), (300, 48, 2, 5, True, (0.1, 1.0, 10.0)), (523, 5, 3, 1, False, (1.0,))]


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as ge
    ge.build()
    return torch.device("cuda:0")


def as_np(t):
    return t.detach().cpu().numpy()


def strided(X, pad, dev):
    """X inside a wider buffer whose pad columns hold NaN: a kernel that reads past d sees it"""
    Xd = torch.from_numpy(X).to(dev)
    if not pad:
        return Xd
    buf = torch.full((X.shape[0], X.shape[1] + pad), float("nan"), device=dev)
    buf[:, :X.shape[1]] = Xd
    return buf[:, :X.shape[1]]


def same_bits(a, b):
    """every tensor field bit for bit (NaN equal to NaN), every other field equal"""
    for name, x, y in zip(a._fields, a, b):
        if isinstance(x, torch.Tensor):
            assert x.dtype == y.dtype and x.shape == y.shape, name
            if x.dtype.is_floating_point:
                it = torch.int64 if x.dtype == torch.float64 else torch.int32
                assert torch.equal(x.contiguous().view(it), y.contiguous().view(it)), name
            else:
                assert torch.equal(x, y), name
        else:
            assert x == y or (x != x and y != y), name


def rows_of(fold, F):
    return np.concatenate([np.flatnonzero(fold == f) for f in range(F)])


def models_of(res, F, L):
    """(m, l, coef, intercept) of every model that has a training set"""
    out = [(F, l, as_np(res.path_coef[l]), as_np(res.path_intercept[l])) for l in range(L)]
    if F > 1:
        out += [(m, l, as_np(res.fold_coef[m, l]), as_np(res.fold_intercept[m, l])) for m in range(F) for l in range(L)]
    return out


# ------------------------------------------------------------------ 1. the first pass
@pytest.mark.parametrize("n, d, c, F, pad", sorted(FIRST_TOL))
def test_first_pass_against_the_fp64_reference(dev, n, d, c, F, pad):
    from gae_dgl_amd import ops
    X, y = R.make_case(n, d, c, seed=n)
    fold = np.arange(n) % F                                            # F = 3: 2 chunks + 1 rows per fold
    lams = [1.0, 2.0] if F > 1 else [1.0]
    res = ops.logreg(strided(X, pad, dev), torch.from_numpy(y).to(dev), lams, folds=F, fold=torch.from_numpy(fold).to(dev),
                     max_iter=1)
    p, rows = as_np(res.pivot), rows_of(fold, F)
    assert np.array_equal(p, as_np(torch.from_numpy(X[rows]).to(dev).mean(0)))
    worst = worst32 = 0.0
    for m, l, coef, icpt in models_of(res, F, len(lams)):
        tr = rows if m == F else rows[fold[rows] != m]
        W64, _, _ = R.fit(X, y, tr, lams[l], c, p, max_iter=1)
        W32, _, _ = R.fit(X, y, tr, lams[l], c, p, max_iter=1, dtype=np.float32)
        scale = np.abs(W64).max()
        worst = max(worst, np.abs(R.from_model(coef, icpt, p) - W64).max() / scale)
        worst32 = max(worst32, np.abs(W32 - W64).max() / scale)
    print(f"device deviation {worst:.3g}, fp32 numpy {worst32:.3g}, tolerance {FIRST_TOL[(n, d, c, F, pad)]:.3g}")
    assert worst <= FIRST_TOL[(n, d, c, F, pad)]
    assert worst <= 16 * worst32
    assert int(res.n_iter.max()) == 1 and res.n_used == n


# ------------------------------------------------------------------ 2., 3. converged fits and their CV tables
@functools.lru_cache(maxsize=None)
def fitted(n, d, c, F, ragged, lams):
    from gae_dgl_amd import ops
    dev = torch.device("cuda:0")
    X, y = R.make_case(n, d, c, seed=n)
    fold = R.deal_folds(n, F, 0, ragged) if F > 1 else np.zeros(n, dtype=np.int64)
    res = ops.logreg(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev), list(lams), folds=F,
                     fold=torch.from_numpy(fold).to(dev), tol=TOL, check_every=8)
    return X, y, fold, res


@pytest.mark.parametrize("n, d, c, F, ragged, lams", FIT_CASES)
def test_every_model_of_a_converged_fit_is_a_minimiser(dev, n, d, c, F, ragged, lams):
    X, y, fold, res = fitted(n, d, c, F, ragged, lams)
    p, rows = as_np(res.pivot), rows_of(fold, F)
    info, conv, n_iter = as_np(res.info), as_np(res.converged), as_np(res.n_iter)
    first = 1 if F == 1 else 0                                         # folds = 1: fold model 0 has no training row
    assert (info[first:] == 0).all() and (conv[first:] == 1).all() and (n_iter[first:] <= 200).all()
    if F == 1:
        assert info[0, 0] == -1 and conv[0, 0] == 0 and n_iter[0, 0] == 0
    worst = [0.0, 0.0, 0.0]
    for m, l, coef, icpt in models_of(res, F, len(lams)):
        tr = rows if m == F else rows[fold[rows] != m]
        W = R.from_model(coef, icpt, p)
        W64, _, conv64 = R.fit(X, y, tr, lams[l], c, p, tol=1e-10, max_iter=5000)
        assert conv64
        step = R.majoriser_step(X, y, tr, lams[l], p, W) / max(1.0, np.abs(W).max())
        J, J64 = R.objective(X, y, tr, lams[l], p, W), R.objective(X, y, tr, lams[l], p, W64)
        total = max(np.abs(coef.sum(0)).max(), abs(icpt.sum()))
        worst = [max(a, b) for a, b in zip(worst, (step / TOL, (J - J64) / J64, total))]
        assert step <= 2 * TOL, (m, l, step)
        assert J <= J64 * (1 + 1e-5), (m, l, J, J64)
        assert total <= 1e-4, (m, l, total)
    print(f"majoriser step / tol {worst[0]:.3g}, J above the optimum by {worst[1]:.3g} relative, class sums {worst[2]:.3g}")
    assert res.n_used == n and as_np(res.fold_counts).tolist() == np.bincount(fold, minlength=F).tolist()
    assert as_np(res.class_counts).tolist() == np.bincount(y, minlength=c).tolist()
    chosen = list(lams).index(res.lam)
    assert np.array_equal(as_np(res.coef), as_np(res.path_coef[chosen]))
    nll_all, _, _ = R.heldout(X, y, rows, as_np(res.coef), as_np(res.intercept))
    assert res.train_logloss == pytest.approx(nll_all / n, rel=1e-5)


@pytest.mark.parametrize("n, d, c, F, ragged, lams", FIT_CASES[:2])
def test_cv_tables_recomputed_at_the_devices_own_coefficients(dev, n, d, c, F, ragged, lams):
    from gae_dgl_amd.ops.ridge import _choose
    X, y, fold, res = fitted(n, d, c, F, ragged, lams)
    rows = rows_of(fold, F)
    cv_nll, cv_correct = as_np(res.cv_nll), as_np(res.cv_correct)
    assert cv_nll.shape == (F, len(lams)) and cv_correct.dtype == np.int64
    left_out = worst = 0
    for m in range(F):
        own = rows[fold[rows] == m]
        for l in range(len(lams)):
            nll, hit, kept = R.heldout(X, y, own, as_np(res.fold_coef[m, l]), as_np(res.fold_intercept[m, l]))
            worst = max(worst, abs(cv_nll[m, l] - nll) / len(own))
            assert abs(cv_nll[m, l] - nll) <= ROW_TOL[(n, d, c)] * len(own)
            # exact on the rows whose top two logits are 1e-4 apart: the others may fall either way
            assert int((hit & kept).sum()) <= cv_correct[m, l] <= int((hit & kept).sum()) + int((~kept).sum())
            left_out += int((~kept).sum())
    print(f"cv_nll off by at most {worst:.3g} per row; {left_out} of {n * len(lams)} rows inside the margin")
    assert left_out <= 0.01 * n * len(lams)
    logloss, acc = as_np(res.cv_logloss), as_np(res.cv_accuracy)
    assert np.allclose(logloss, cv_nll.sum(0) / n, rtol=1e-15, atol=0) and np.allclose(acc, cv_correct.sum(0) / n, rtol=1e-15)
    ok = [bool((as_np(res.info)[:, l] == 0).all()) for l in range(len(lams))]
    assert res.lam == lams[_choose(ok, logloss.tolist())] and as_np(res.lambdas).tolist() == list(lams)


# ------------------------------------------------------------------ 4. never read; the same bits
def test_rows_that_are_not_listed_are_never_read(dev):
    from gae_dgl_amd import ops
    n, d, c, F = 700, 16, 7, 3
    X, y = R.make_case(n, d, c, seed=n)
    rng = np.random.default_rng(3)
    fold = R.deal_folds(n, F, 1)
    y = y.copy()
    y[rng.choice(n, 60, replace=False)] = -1                           # unlabelled
    fold[rng.choice(n, 90, replace=False)] = -1                        # a test set
    keep = (y >= 0) & (fold >= 0)
    Xp = X.copy()
    Xp[~keep] = np.where(rng.random((int((~keep).sum()), d)) < 0.5, np.nan, np.inf)
    kw = dict(folds=F, tol=TOL, max_iter=200, n_classes=c)
    a = ops.logreg(torch.from_numpy(Xp).to(dev), torch.from_numpy(y).to(dev), [0.1, 10.0], fold=torch.from_numpy(fold).to(dev), **kw)
    b = ops.logreg(torch.from_numpy(X[keep]).to(dev), torch.from_numpy(y[keep]).to(dev), [0.1, 10.0],
                   fold=torch.from_numpy(fold[keep]).to(dev), **kw)
    same_bits(a, b)
    assert a.n_used == int(keep.sum()) < n and bool(a.converged.all()) and bool(torch.isfinite(a.coef).all())


def test_same_bits_for_any_stride_check_cut_company_and_stream(dev):
    from gae_dgl_amd import ops
    n, d, c, F = 700, 16, 7, 3
    X, y = R.make_case(n, d, c, seed=n)
    yd, fd = torch.from_numpy(y).to(dev), torch.from_numpy(R.deal_folds(n, F)).to(dev)
    lams = [0.1, 1.0, 10.0]
    kw = dict(folds=F, fold=fd, tol=TOL, max_iter=200)
    base = ops.logreg(strided(X, 0, dev), yd, lams, **kw)
    assert bool(base.converged.all())
    same_bits(base, ops.logreg(strided(X, 0, dev), yd, lams, **kw))                    # run to run
    same_bits(base, ops.logreg(strided(X, 8, dev), yd, lams, **kw))                    # ldx = d + 8
    for every in (1, 1000):
        same_bits(base, ops.logreg(strided(X, 0, dev), yd, lams, check_every=every, **kw))
    for batch in (1, 4):
        same_bits(base, ops.logreg(strided(X, 0, dev), yd, lams, model_batch=batch, **kw))
    alone = ops.logreg(strided(X, 0, dev), yd, [1.0], **kw)                             # one lambda alone
    for name in ("fold_coef", "fold_intercept", "cv_nll", "cv_correct", "n_iter", "converged", "info"):
        x, z = getattr(alone, name), getattr(base, name)
        assert torch.equal(x[:, 0], z[:, 1]), name
    assert torch.equal(alone.coef, base.path_coef[1]) and torch.equal(alone.intercept, base.path_intercept[1])
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other = ops.logreg(strided(X, 0, dev), yd, lams, **kw)
    side.synchronize()
    same_bits(base, other)


def test_a_list_long_enough_for_the_64_lane_order_of_partials(dev):
    from gae_dgl_amd import ops
    n, d, c, F = 70000, 16, 3, 2
    X, y = R.make_case(n, d, c, seed=7)
    fold = np.arange(n) % F
    Xd, yd, fd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(fold).to(dev)
    a = ops.logreg(Xd, yd, [1.0], folds=F, fold=fd, max_iter=20, tol=0.0)
    b = ops.logreg(Xd, yd, [1.0], folds=F, fold=fd, max_iter=20, tol=0.0)
    same_bits(a, b)
    slabs = -(-(-(-n // C) + F) // ops.LOGREG_SLAB_CHUNKS)
    assert slabs > 32 and as_np(a.n_iter).tolist() == [[20], [20], [20]] and not bool(a.converged.any())
    p, rows = as_np(a.pivot), np.arange(n)
    for m, l, coef, icpt in models_of(a, F, 1):
        tr = rows if m == F else rows[fold != m]
        J = R.objective(X, y, tr, 1.0, p, R.from_model(coef, icpt, p))
        J0 = len(tr) * np.log(c)
        print(f"model {m}: J = {J:.8g} after 20 passes, {J0:.8g} at W = 0")
        assert J < J0


# ------------------------------------------------------------------ 5. predict, errors, the surface
def test_predict_labels_probabilities_and_non_finite_rows(dev):
    from gae_dgl_amd import ops
    n, d, c, F, ragged, lams = FIT_CASES[0]
    X, y, fold, res = fitted(n, d, c, F, ragged, lams)
    Xq = np.concatenate([X, R.make_case(133, d, c, seed=5)[0]])       # 833 rows: 13 blocks and a rest
    Xq[17, 3], Xq[800, 0] = np.nan, -np.inf
    Xd = strided(Xq, 8, dev)
    status = torch.zeros(4, dtype=torch.int64, device=dev)
    labels, proba = ops.logreg_predict(Xd, res.coef, res.intercept, res.pivot, proba=True, status=status)
    assert labels.dtype == torch.int32 and proba.dtype == torch.float32 and proba.shape == (833, c)
    labels, proba = as_np(labels), as_np(proba)
    bad = np.zeros(833, dtype=bool); bad[[17, 800]] = True
    assert (labels[bad] == -1).all() and np.isnan(proba[bad]).all() and as_np(status).tolist() == [0, 2, 0, 0]
    Z = Xq[~bad].astype(np.float64) @ as_np(res.coef).T + as_np(res.intercept)
    top = np.sort(Z, 1)
    kept = top[:, -1] - top[:, -2] >= 1e-4
    assert (~kept).sum() <= 0.01 * len(Z) and np.array_equal(labels[~bad][kept], Z.argmax(1)[kept])
    P = np.exp(Z - Z.max(1, keepdims=True)); P /= P.sum(1, keepdims=True)
    err = np.abs(proba[~bad] - P).max()
    Z32 = (Xq[~bad] - as_np(res.pivot)) @ as_np(res.coef).T.astype(np.float32) \
        + (as_np(res.intercept) + as_np(res.coef) @ as_np(res.pivot).astype(np.float64)).astype(np.float32)
    err32 = np.abs(R.softmax_rows(Z32) - P).max()                      # the same model in fp32 numpy: the yardstick
    print(f"max |p - p64| = {err:.3g}, fp32 numpy {err32:.3g}, tolerance {PROBA_TOL:.3g}")
    assert err <= PROBA_TOL and err <= 16 * err32 and np.allclose(proba[~bad].sum(1), 1.0, atol=1e-6)
    assert np.array_equal(as_np(res.predict(Xd)), labels) and np.array_equal(as_np(res.predict_proba(Xd)), proba, equal_nan=True)
    lin = res.to_torch()
    with torch.no_grad():
        q = torch.softmax(lin(torch.from_numpy(Xq[~bad]).to(dev)), 1)
    assert np.abs(as_np(q) - proba[~bad]).max() <= 1e-5


def test_non_finite_listed_rows_and_shapes_over_a_limit_raise(dev):
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    X, y = R.make_case(300, 6, 3, seed=2)
    Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
    for v in (float("nan"), float("inf")):
        bad = Xd.clone(); bad[41, 2] = v
        with pytest.raises(GaeHipError, match="1 of the 300 listed rows hold non-finite values"):
            ops.logreg(bad, yd, [1.0], folds=3)
        yy = yd.clone(); yy[41] = -1                                   # ... unless the row is not listed
        assert bool(torch.isfinite(ops.logreg(bad, yy, [1.0], folds=3).coef).all())
    wide = torch.randn(50, 129, device=dev)
    with pytest.raises(GaeHipError, match="d = 129 outside 1..128"):
        ops.logreg_predict(wide, torch.zeros(2, 129, device=dev), torch.zeros(2, device=dev))
    with pytest.raises(GaeHipError, match="c = 33 outside 2..32"):
        ops.logreg_predict(Xd, torch.zeros(33, 6, device=dev), torch.zeros(33, device=dev))
    with pytest.raises((GaeHipError, ValueError)):
        ops.logreg(wide, torch.arange(50, device=dev) % 2)
    with pytest.raises((GaeHipError, ValueError)):
        ops.logreg(Xd, torch.arange(300, device=dev) % 33)
    with pytest.raises(GaeHipError):
        ops.logreg(Xd.double(), yd)


def planted_graph(n, k, dev, seed=0):
    import gae_dgl_amd as G
    rng = np.random.default_rng(seed)
    comm = rng.integers(0, k, n)
    a, b = rng.integers(0, n, 6000), rng.integers(0, n, 6000)
    keep = (comm[a] == comm[b]) & (a != b)
    a, b = a[keep], b[keep]
    feats = np.eye(k, dtype=np.float32)[comm] + 0.5 * rng.standard_normal((n, k)).astype(np.float32)
    def fresh():
        g = G.DGLGraph()
        g.add_nodes(n)
        g.add_edges(np.concatenate([a, b]), np.concatenate([b, a]))
        g.to(dev)
        g.ndata['h'] = torch.from_numpy(feats).to(dev)
        return g
    return fresh, comm, (a, b, feats)


def test_classify_nodes_is_logreg_of_the_embedding(dev):
    import gae_dgl_amd as G
    from gae_dgl_amd import ops
    from gae_dgl_amd.vgae import VGAE
    fresh, comm, _ = planted_graph(300, 3, dev)
    labels = torch.from_numpy(comm).to(dev)
    labels[:20] = -1
    kw = dict(lambdas=[0.1, 1.0, 10.0], folds=3, seed=2, tol=TOL)
    torch.manual_seed(0)
    model = G.GAE(3, [32, 16]).to(dev).eval()
    g = fresh()
    feat = g.ndata['h']
    res = model.classify_nodes(g, labels, **kw)
    assert g.ndata['h'] is feat and res.n_used == 280 and res.coef.shape == (3, 16)
    with torch.no_grad():
        same_bits(res, ops.logreg(model.encode(fresh()), labels, **kw))
    torch.manual_seed(0)
    vg = VGAE(3, [32, 16]).to(dev).eval()
    with torch.no_grad():
        mu, _ = vg.encode(fresh())
    same_bits(vg.classify_nodes(fresh(), labels, **kw), ops.logreg(mu.contiguous(), labels, **kw))


def test_logreg_graphs_is_logreg_of_the_molecule_features(dev):
    import gae_dgl_amd as G
    from gae_dgl_amd import ops
    from gae_dgl_amd.dataset import DeviceGraphDataset
    data = DeviceGraphDataset.synthetic_zinc(600, seed=1, device=dev)
    torch.manual_seed(0)
    model = G.GAE(39, [32, 16]).to(dev).eval()
    y = torch.randint(0, 3, (600,), generator=torch.Generator().manual_seed(2)).to(dev)
    kw = dict(lambdas=[1.0, 100.0], folds=4, seed=3, max_iter=50)
    want = ops.logreg(model.embed_graphs(data), y, **kw)
    same_bits(model.logreg_graphs(data, y, fused="auto", batch_size=256, **kw), want)
    assert want.coef.shape == (3, 48) and want.n_used == 600
    with pytest.raises(ValueError):
        model.logreg_graphs(data, y, grad=True)


def test_cli_embed_logreg(tmp_path, capsys):
    from gae_dgl_amd import embed as E
    import gae_dgl_amd as G
    torch.manual_seed(0)
    ckpt = str(tmp_path / "m.pkl")
    torch.save(G.GAE(39, [32, 16]).state_dict(), ckpt)
    ng = 300
    y = np.random.default_rng(1).integers(0, 2, ng)
    y[:7] = -1
    np.save(tmp_path / "y.npy", y)
    E.main(["--checkpoint", ckpt, "--hidden_dims", "32", "16", "--synthetic", str(ng), "--out", str(tmp_path / "f.npy"),
            "--logreg", "1", "100", "10000", "--logreg_folds", "3", "--logreg_out", str(tmp_path / "model.npz"),
            "--labels", str(tmp_path / "y.npy")])
    text = capsys.readouterr().out
    assert f"Fitted logistic regression on {ng - 7} molecules, 2 classes, 3 lambdas x 3 folds" in text
    line = [l for l in text.splitlines() if l.startswith("LogReg (3-fold CV, lambda = ")]
    assert len(line) == 1 and " accuracy: " in line[0] and " | macro-F1: " in line[0] and " | log-loss: " in line[0], text
    z = np.load(tmp_path / "model.npz")
    res, cm = E.main.logreg, E.main.logreg_scores
    assert sorted(z.files) == ["coef", "cv_accuracy", "cv_logloss", "intercept", "lam", "lambdas", "pivot"]
    assert z["coef"].shape == (2, 48) and z["coef"].dtype == np.float64 and z["lambdas"].tolist() == [1.0, 100.0, 10000.0]
    assert np.array_equal(z["coef"], as_np(res.coef)) and np.array_equal(z["intercept"], as_np(res.intercept))
    assert float(z["lam"]) == res.lam and f"lambda = {res.lam:g})" in line[0]
    chosen = z["lambdas"].tolist().index(float(z["lam"]))
    # the pooled held-out predictions are the CV table's
    assert cm["n"] == ng - 7 and cm["accuracy"] == pytest.approx(float(z["cv_accuracy"][chosen]), abs=0.01 + 1e-12)
    assert cm["log_loss"] == pytest.approx(float(z["cv_logloss"][chosen]), rel=1e-4)
    assert f"accuracy: {cm['accuracy']:.4f} | macro-F1: {cm['macro_f1']:.4f} | log-loss: {cm['log_loss']:.4f}" in line[0]


def test_cli_train_transductive_classify(tmp_path, capsys):
    from gae_dgl_amd import train_transductive as TT
    n, k = 300, 3
    _, comm, (a, b, feats) = planted_graph(n, k, torch.device("cuda:0"))
    classes = comm.copy(); classes[:10] = -1
    os.makedirs(tmp_path / "data", exist_ok=True)
    np.savez(tmp_path / "data" / "cora.npz", src=np.concatenate([a, b]), dst=np.concatenate([b, a]), features=feats, n=n,
             labels=classes)
    out = tmp_path / "model.npz"
    TT.main(["--dataset", "cora", "--data_root", str(tmp_path / "data"), "-e", "20", "-s", str(tmp_path), "--seed", "0",
             "--log_every", "1000", "--classify", "0.1", "1", "10", "--classify_folds", "3", "--classify_test_frac", "0.25",
             "--classify_seed", "1", "--classify_out", str(out)])
    text = capsys.readouterr().out
    line = [l for l in text.splitlines() if l.startswith("LogReg (3-fold CV, lambda = ")]
    assert len(line) == 1 and " test accuracy: " in line[0] and " | macro-F1: " in line[0] and " | log-loss: " in line[0], text
    z = np.load(out)
    last = TT.main.last_classify
    assert z["coef"].shape == (3, 16) and z["coef"].dtype == np.float64 and z["intercept"].shape == (3,)
    assert z["lambdas"].tolist() == [0.1, 1.0, 10.0] and float(z["lam"]) == last["result"].lam
    n_test = round(0.25 * (n - 10))
    assert z["test_index"].shape == (n_test,) and z["test_pred"].dtype == np.int32 and (classes[z["test_index"]] >= 0).all()
    assert last["result"].n_used == n - 10 - n_test and last["metrics"]["n"] == n_test
    acc = float((z["test_pred"] == classes[z["test_index"]]).mean())
    assert acc == pytest.approx(last["metrics"]["accuracy"]) and f"test accuracy: {acc:.4f}" in line[0]
    assert acc > 0.6                                                   # three planted communities: chance is 1 / 3
