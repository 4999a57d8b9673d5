"""K30 without a GPU: the numpy restatement tests/boost_ref.py is checked against itself (it is the yardstick of
tests/test_gpu_boost.py) -- the restated sigma against a long-double sigmoid, the histogram split against an exhaustive
search, monotone training error, the XOR target a linear model cannot learn -- and the C entry points and ops.boost reject
bad arguments before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import boost_ref as B


def test_restated_sigma_against_the_long_double_sigmoid():
    """The bound.  The degree-13 Taylor polynomial on |r| <= ln 2 / 2 leaves r^14 / 14! <= 0.3466^14 / 8.7e10 = 4.2e-18
    relative to exp(r) >= 0.707: 0.06 units of 2^-53.  Rounding: the reduction r = (t - k hi) - k lo is exact in its first
    product (hi has 21 trailing zero bits, k < 2^6) and loses at most 2^-53 |r| twice, which moves exp(r) by 2 |r| 2^-53
    <= 0.7 units; the Horner steps each round twice, and step j's error reaches the result scaled by |r|^j: 2 (1/2) (1 +
    0.35 + 0.35^2 + ..) <= 1.6 units of 2^-53 with the units of exp(r) in [0.707, 1.414] counted at their worst; the scaling
    by 2^k is exact; 1 + e, the division and (for F >= 0) 1 - q round once each, half a unit of their results, and the
    results are >= 1/2: 1.5 units.  Together below 4.4 units: the test holds sigma at 4.5 units of 2^-53 relative."""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps      # the yardstick is wider than what it measures
    x = np.concatenate([np.linspace(-40.0, 40.0, 400001), np.random.default_rng(0).uniform(-40, 40, 200000),
                        [0.0, -0.0, 40.0, -40.0, np.nextafter(40.0, 0), -np.nextafter(40.0, 0)]])
    want = 1 / (1 + np.exp(-x.astype(np.longdouble)))
    err = np.abs((B.sigma(x) - want) / want) / np.longdouble(2.0 ** -53)
    print(f"sigma: max error {float(err.max()):.3f} units of 2^-53 at x = {x[int(err.argmax())]}")
    assert float(err.max()) <= 4.5
    # the clamp: beyond 40 the value of 40, 1 - q rounds to exactly 1 above, q = sigma(-40) below; a NaN takes the clamp
    assert B.sigma(np.array([40.0, 55.0, 1e300]))[0] == 1.0 and (B.sigma(np.array([55.0, 1e300, np.inf])) == 1.0).all()
    low = B.sigma(np.array([-40.0, -41.0, -1e300, -np.inf]))
    assert (low == low[0]).all() and 4.2e-18 < low[0] < 4.3e-18
    assert B.sigma(np.array([0.0]))[0] == 0.5
    # exp_neg itself, against exp in long double
    a = np.linspace(0.0, 40.0, 100001)
    e = np.exp(-a.astype(np.longdouble))
    assert float(np.abs((B.exp_neg(a) - e) / e).max() / 2.0 ** -53) <= 3.0


def test_histogram_split_equals_an_exhaustive_search():
    rng = np.random.default_rng(3)
    X = rng.integers(0, 5, size=(8, 2)).astype(np.float32)
    y = rng.normal(size=8).astype(np.float32)
    lam, lr = 0.5, 1.0
    m = B.boost(X, y, "squared", 1, max_depth=1, learning_rates=(lr,), lambdas=(lam,), folds=1, max_bins=8)
    g = m.base_score - y.astype(np.float64)                             # F - y at the start
    best = (-np.inf, None, None)
    for f in range(2):
        for thr in m.edges[f, :m.n_edges[f]]:                           # every code threshold, ascending: ties keep the first
            L = X[:, f] <= thr
            if L.sum() < 1 or (~L).sum() < 1:
                continue
            s = g[L].sum() ** 2 / (L.sum() + lam) + g[~L].sum() ** 2 / ((~L).sum() + lam)
            if s > best[0]:
                best = (s, f, thr)
    parent = g.sum() ** 2 / (8 + lam)
    assert best[0] > parent and m.feature[0, 0] == best[1] and m.threshold[0, 0] == best[2]
    assert m.gain[0, 0] == pytest.approx(best[0] - parent, rel=1e-6)
    L = X[:, best[1]] <= best[2]
    assert m.count[0, 1] == L.sum() and m.count[0, 2] == 8 - L.sum()
    assert m.value[0, 1] == pytest.approx(-lr * g[L].sum() / (L.sum() + lam), rel=1e-6)
    assert m.value[0, 2] == pytest.approx(-lr * g[~L].sum() / ((~L).sum() + lam), rel=1e-6)


def test_squared_training_error_never_rises():
    rng = np.random.default_rng(4)
    X = rng.normal(size=(200, 4)).astype(np.float32)
    y = (np.sin(X[:, 0]) + X[:, 1] * X[:, 2]).astype(np.float32)
    m = B.boost(X, y, "squared", 15, max_depth=3, learning_rates=(0.5,), lambdas=(0.0,), folds=1)
    errs = [float(((B.predict(m, X, n_rounds=r) - y) ** 2).sum()) for r in range(16)]
    assert all(b <= a for a, b in zip(errs, errs[1:])) and errs[-1] < 0.2 * errs[0]
    assert np.array_equal(B.predict(m, X, n_rounds=15), m.train_score)


def test_xor_is_learnt_where_a_linear_model_is_not():
    rng = np.random.default_rng(0)
    X = rng.normal(size=(600, 2)).astype(np.float32)
    y = (X[:, 0] * X[:, 1] > 0).astype(np.int64)
    m = B.boost(X, y, "logistic", 20, max_depth=2, learning_rates=(0.3,), max_bins=32, folds=5, seed=0)
    fold, right = B.default_fold(600, 5, 0), 0
    for k in range(5):                                                 # least squares on +-1 targets, the same folds
        tr = fold != k
        A = np.c_[X, np.ones(600)]
        w = np.linalg.lstsq(A[tr], 2.0 * y[tr] - 1, rcond=None)[0]
        right += int(((A[~tr] @ w > 0) == (y[~tr] == 1)).sum())
    print(f"boost held-out accuracy {m.cv_accuracy:.4f}, linear {right / 600:.4f}")
    assert m.cv_accuracy >= 0.9
    assert right / 600 <= 0.65


def test_selection_rule_ties_and_eligibility():
    curve = np.array([[3.0, 1.0, 1.0], [1.0, 0.5, 0.5], [0.5, 0.25, np.nan]])
    assert B.choose(curve, [True, True, False]) == (1, 1)
    assert B.choose(curve, [True, False, False]) == (0, 1)
    assert B.choose(curve, [True, True, True]) == (2, 1)
    assert B.choose(curve, [False, False, False]) == (-1, -1)


def lib():
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    return _lib.load()


def test_workspace_query_accepts_the_limits_and_rejects_one_past_each():
    q = lib().gae_boost_workspace_bytes
    order = ["n_used", "d", "max_bins", "max_depth", "folds", "n_cfg"]
    ok = dict(n_used=1000, d=256, max_bins=256, max_depth=8, folds=5, n_cfg=3)
    assert q(*[ok[k] for k in order]) > 0
    assert q(1, 1, 2, 1, 0, 1) > 0 and q(1000, 48, 64, 4, 255, 1) > 0 and q(1000, 48, 64, 4, 0, 256) > 0
    for name, bad in (("d", 257), ("d", 0), ("max_bins", 257), ("max_bins", 1), ("max_depth", 9), ("max_depth", 0),
                      ("folds", 1), ("folds", -1), ("folds", 256), ("n_cfg", 0), ("n_cfg", 43), ("n_used", 0),
                      ("n_used", 2 ** 31), ("n_used", -1)):
        args = dict(ok, **{name: bad})
        assert q(*[args[k] for k in order]) < 0, (name, bad)
    base = q(1000, 48, 64, 4, 5, 3)
    assert q(2000, 48, 64, 4, 5, 3) > base                              # grows with n
    assert q(1000, 48, 64, 4, 5, 6) > base and q(1000, 48, 64, 4, 9, 3) > base      # and with the models
    assert q(1000, 48, 64, 5, 5, 3) > base                              # the per-round scratch (tables, lists) with the depth
    # no argument for the rounds: the scratch does not depend on them (the kept tables are the caller's outputs)


def test_entry_points_reject_bad_arguments_before_any_launch():
    L = lib()
    E_NULL, E_SIZE, E_RANGE = -1, -2, -6

    def fit(n_used=8, d=4, bins=8, folds=2, objective=0, base=0.0, exponent=0, lr=(0.1,), lam=(1.0,), R=5, depth=3, m=4, msl=1,
            mcw=1.0, min_gain=0.0, check=16, ws_bytes=1 << 30):
        k = len(lr)
        return L.gae_boost_fit(None, None, None, n_used, d, bins, None, None, folds, objective, base, exponent,
                               (ctypes.c_double * k)(*lr), (ctypes.c_double * k)(*lam), k, R, depth, m, msl, mcw, min_gain, 0,
                               check, None, None, None, None, None, None, None, None, None, None, None, None, None, None,
                               ws_bytes, None)
    assert fit() == E_NULL and b"NULL" in L.gae_last_error()           # everything else is in order: the NULL arrays
    for kw in (dict(n_used=0), dict(d=257), dict(d=0), dict(bins=257), dict(bins=1), dict(depth=9), dict(depth=0), dict(R=4097),
               dict(R=0), dict(folds=1), dict(folds=255, lr=(0.1, 0.2), lam=(1.0, 1.0)), dict(objective=2), dict(m=5), dict(m=0),
               dict(msl=0), dict(check=0), dict(lr=(0.0,)), dict(lr=(1.5,)), dict(lr=(float("nan"),)), dict(lam=(-1.0,)),
               dict(lam=(float("inf"),)), dict(mcw=-1.0), dict(min_gain=float("nan")), dict(base=float("inf")),
               dict(exponent=201)):
        assert fit(**kw) in (E_SIZE, E_RANGE), kw
    assert fit(mcw=0.0, lam=(0.0,)) == E_RANGE and b"divide by zero" in L.gae_last_error()
    assert fit(mcw=0.0, lam=(1e-3,)) == E_NULL and fit(mcw=1e-3, lam=(0.0,)) == E_NULL
    assert fit(lr=(1.0,)) == E_NULL

    def predict(ldx=4, m=8, d=4, R=3, cap=15):
        return L.gae_boost_predict(None, ldx, m, d, R, cap, None, None, None, None, 0.0, None, None, None)
    assert predict() == E_NULL and b"NULL" in L.gae_last_error()
    for kw in (dict(m=-1), dict(ldx=3), dict(d=0), dict(d=257), dict(R=4097), dict(R=-1), dict(cap=0), dict(cap=512)):
        assert predict(**kw) in (E_SIZE, E_RANGE), kw


def test_the_wrapper_rejects_bad_arguments_without_a_gpu():
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    X, y = torch.zeros(20, 4), torch.zeros(20)
    labels = torch.zeros(20, dtype=torch.int64)
    bad = (ValueError, GaeHipError)
    for kw in (dict(max_depth=9), dict(max_depth=0), dict(max_bins=257), dict(max_bins=1), dict(n_rounds=4097), dict(n_rounds=0),
               dict(learning_rates=(0.0,)), dict(learning_rates=(1.5,)), dict(lambdas=(-1.0,)), dict(min_child_weight=-1.0),
               dict(min_child_weight=0.0, lambdas=(1.0, 0.0)), dict(min_samples_leaf=0), dict(min_gain=-1.0),
               dict(max_features=0), dict(max_features=1.5), dict(folds=0), dict(folds=256), dict(check_every=0),
               dict(folds=50, learning_rates=(0.1, 0.2, 0.3), lambdas=(1.0, 2.0)),          # 51 x 6 = 306 models
               dict(folds=1, learning_rates=(0.1, 0.2)), dict(objective="hinge"), dict(seed=-1), dict(max_depth=4.0)):
        with pytest.raises(bad):
            ops.boost(X, y, **dict(dict(n_rounds=5), **kw))
    with pytest.raises(bad):
        ops.boost(torch.zeros(20, 257), y)                              # d one past the limit
    with pytest.raises(bad):
        ops.boost(X.double(), y)                                        # misplaced dtypes
    with pytest.raises(bad):
        ops.boost(X, y.double())
    with pytest.raises(bad):
        ops.boost(X, labels)                                            # int targets with "squared"
    with pytest.raises(bad):
        ops.boost(X, y, "logistic")                                     # float labels with "logistic"
    with pytest.raises(bad):
        ops.boost(X, labels == 1, "logistic")
    with pytest.raises(bad):
        ops.boost(X, torch.zeros(20, 2))                                # one target
    with pytest.raises(bad):
        ops.boost(X, labels + 2, "logistic")                            # labels outside {0, 1}
    with pytest.raises(bad):
        ops.boost(X, labels - 2, "logistic")
    with pytest.raises(bad):
        ops.boost(X, y, fold=torch.full((20,), 5))                      # a fold id outside -1..folds-1
    with pytest.raises(GaeHipError, match="no CPU fallback"):
        ops.boost(X, y)                                                 # everything in order: only the device is missing
