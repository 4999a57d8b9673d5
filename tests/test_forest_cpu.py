"""K26 without a GPU: the numpy restatement tests/forest_ref.py is checked against itself (it is the yardstick of
tests/test_gpu_forest.py) -- exact CART splits on lossless bins, training targets reproduced to the quantisation step, the
Philox bootstrap against the scalar Philox of tests/sampled_ref.py, the tie rules, constant targets and columns -- and the
C entry points and ops.forest reject bad arguments before any launch."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import forest_ref as R
import sampled_ref


def paths(model, tree, X):
    """node -> rows of X that pass through it"""
    through = {}
    for i, x in enumerate(X):
        node = 0
        while True:
            through.setdefault(node, []).append(i)
            f = model.feature[tree, node]
            if f < 0:
                break
            node = model.left[tree, node] + (0 if x[f] <= model.threshold[tree, node] else 1)
    return through


def exact_gain(yl, yr):
    """variance-reduction numerator in exact arithmetic: S_L^2 / n_L + S_R^2 / n_R - S^2 / n"""
    sl, sr = sum(yl), sum(yr)
    return sl * sl / len(yl) + sr * sr / len(yr) - (sl + sr) ** 2 / (len(yl) + len(yr))


def test_philox_and_bootstrap_against_the_scalar_philox():
    seed, n_used = 12345, 1000
    key = seed ^ R.KEY_XOR
    words = R.philox(np.arange(5), 3, key)
    for c in range(5):
        assert words[:, c].tolist() == sampled_ref.philox4x32_10(c, 3, key)
    for tree in (0, 7):
        got = R.bootstrap_rows(tree, 37, n_used, seed)
        want = [(sampled_ref.philox4x32_10(j >> 2, tree, key)[j & 3] * n_used) >> 32 for j in range(37)]
        assert got.tolist() == want
    assert R.KEY_XOR != sampled_ref.KEY_XOR
    sel = R.feature_subset(2, 5, 10, 3, seed)
    r = [sampled_ref.philox4x32_10((5 << 8) | f, (1 << 32) + 2, key)[0] for f in range(10)]
    assert sorted(np.nonzero(sel)[0].tolist()) == sorted(sorted(range(10), key=lambda f: (r[f], f))[:3])
    assert R.feature_subset(2, 5, 10, 10, seed).all()


@pytest.mark.parametrize("seed", [0, 1])
def test_splits_equal_a_brute_force_cart_search_on_lossless_bins(seed):
    rng = np.random.default_rng(seed)
    n, d, bins = 120, 4, 8
    X = rng.integers(0, bins, size=(n, d)).astype(np.float32)
    y = rng.integers(-20, 21, size=n).astype(np.float32)
    m = R.forest(X, y, 1, max_depth=5, max_bins=bins, bootstrap=False)
    assert (m.n_edges <= bins - 1).all() and m.codes.max() < bins
    for f in range(d):                                                 # lossless: one code per distinct value
        assert len(np.unique(m.codes[:, f])) == len(np.unique(X[:, f]))
    through = paths(m, 0, X)
    yf = [Fraction(int(v)) for v in y]
    n_split = 0
    for node, rows in through.items():
        assert m.count[0, node] == len(rows)
        best = Fraction(0)
        for f in range(d):
            for thr in np.unique(X[rows, f])[:-1]:
                left = [i for i in rows if X[i, f] <= thr]
                right = [i for i in rows if X[i, f] > thr]
                best = max(best, exact_gain([yf[i] for i in left], [yf[i] for i in right]))
        if m.feature[0, node] < 0:
            depth = 0
            k = node
            while k:                                                   # a leaf below the depth limit has nothing to gain
                k = int(np.nonzero((m.left[0] == k) | (m.left[0] + 1 == k))[0][0])
                depth += 1
            assert depth == 5 or best == 0
            continue
        n_split += 1
        f, thr = m.feature[0, node], m.threshold[0, node]
        left = [i for i in rows if X[i, f] <= thr]
        right = [i for i in rows if X[i, f] > thr]
        assert exact_gain([yf[i] for i in left], [yf[i] for i in right]) == best and best > 0
        scale = 4.0 ** -m.exponent[0]                                   # gain is in the units of y^2
        assert abs(m.gain[0, node] - float(best)) <= 1e-9 * max(1.0, float(best))
        assert scale > 0
    assert n_split >= 8


def test_training_targets_are_reproduced_to_the_quantisation_step():
    rng = np.random.default_rng(3)
    n, d = 64, 3
    X = np.stack([rng.permutation(n) for _ in range(d)], 1).astype(np.float32)      # distinct rows, 64 levels
    # targets at least 1/8 of a unit apart over a range of ~ 8 .. 24: two samples differ by >= 2^22 fixed-point steps, their
    # gain (>= 2^43 in step^2) is far above the rounding of the fp64 scores (S^2 / n <= 2^71, half an ulp 2^18), so every
    # pair is split.  (Targets closer than ~ 2^5 steps may stay together in a leaf: best > parent is tested in fp64.)
    y = np.stack([rng.permutation(n) / 8.0, rng.permutation(n) * 0.37], 1).astype(np.float32)
    m = R.forest(X, y, 1, max_depth=16, max_bins=64, bootstrap=False)
    pred = R.predict(m, X)
    step = np.array([2.0 ** -e for e in m.exponent])
    assert (np.abs(pred - y.astype(np.float64)) <= step).all()
    leaves = m.feature[0, :m.n_nodes[0]] < 0
    assert (m.count[0, :m.n_nodes[0]][leaves] == 1).all() and m.n_nodes[0] == 2 * n - 1
    assert np.isnan(m.oob_prediction).all() and np.isnan(m.oob_r2).all()


def test_ties_go_to_the_lower_feature_then_the_lower_bin():
    x = np.array([0, 1, 2, 3], np.float32)
    X = np.stack([x, x, x[::-1]], 1)
    y = np.array([0, 1, 1, 0], np.float32)                            # b = 0 and b = 2 tie, on every column
    m = R.forest(X, y, 1, max_depth=1, max_bins=4, bootstrap=False)
    assert m.feature[0, 0] == 0 and m.threshold_bin[0, 0] == 0 and m.threshold[0, 0] == 0.5
    assert m.left[0, 0] == 1 and m.count[0, :3].tolist() == [4, 1, 3] and m.n_nodes[0] == 3
    m = R.forest(X[:, ::-1].copy(), y, 1, max_depth=1, max_bins=4, bootstrap=False)
    assert m.feature[0, 0] == 0 and m.threshold_bin[0, 0] == 0         # the reversed column first: still f = 0, b = 0


def test_constant_targets_and_constant_columns():
    rng = np.random.default_rng(5)
    X = rng.normal(size=(50, 4)).astype(np.float32)
    m = R.forest(X, np.full(50, 2.5, np.float32), 3, max_depth=6, seed=1)
    assert m.n_nodes.tolist() == [1, 1, 1] and (m.feature[:, 0] == -1).all() and (m.value[:, 0, 0] == 2.5).all()
    assert m.exponent == [0] and (m.importances == 0).all()
    X[:, 1] = 7.0
    y = (X[:, 0] + X[:, 1] + 0.1 * X[:, 2]).astype(np.float32)
    m = R.forest(X, y, 4, max_depth=6, max_features=2, seed=2)
    assert m.n_edges[1] == 0 and not (m.feature == 1).any() and m.n_nodes.min() > 1
    assert m.importances[1] == 0 and abs(m.importances.sum() - 1) < 1e-12


def test_bins_from_order_statistics_are_deduplicated_and_ascending():
    rng = np.random.default_rng(6)
    X = np.stack([rng.normal(size=500), np.repeat(np.arange(5), 100), np.where(rng.random(500) < 0.9, 0.0, rng.normal(size=500))],
                 1).astype(np.float32)
    edges, n_edges = R.make_edges(X, 16)
    assert n_edges[0] == 15 and n_edges[1] == 4 and 1 <= n_edges[2] < 15
    for f in range(3):
        e = edges[f, :n_edges[f]]
        assert (np.diff(e) > 0).all() and np.isinf(edges[f, n_edges[f]:]).all()
    assert edges[1, :4].tolist() == [0.5, 1.5, 2.5, 3.5]
    a = np.float32(1.0)
    b = np.nextafter(a, np.float32(2))
    e2, k2 = R.make_edges(np.array([[a], [b]], np.float32), 4)          # adjacent floats: the edge is a itself
    assert k2[0] == 1 and e2[0, 0] == a
    codes = R.make_codes(X, edges, n_edges)
    assert codes[:, 1].tolist() == np.repeat(np.arange(5), 100).tolist()


# ---- the C entry points without a GPU
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    return _lib.load()


def test_workspace_query_accepts_the_limits_and_rejects_one_past_each():
    q = lib().gae_forest_workspace_bytes
    ok = dict(n_used=1000, d=256, t=8, n_trees=1024, n_boot=1000, max_depth=16, max_bins=256)
    order = ["n_used", "d", "t", "n_trees", "n_boot", "max_depth", "max_bins"]
    assert q(*[ok[k] for k in order]) > 0
    assert q(2 ** 31 - 1, 1, 1, 1, 2 ** 31 - 1, 1, 2) > 0
    assert q(1, 1, 1, 1, 1, 1, 2) > 0
    for name, bad in (("d", 257), ("d", 0), ("t", 9), ("t", 0), ("n_trees", 1025), ("n_trees", 0), ("max_depth", 17),
                      ("max_depth", 0), ("max_bins", 257), ("max_bins", 1), ("n_used", 2 ** 31), ("n_used", 0),
                      ("n_boot", 2 ** 31), ("n_boot", 0), ("n_used", -1)):
        args = dict(ok, **{name: bad})
        assert q(*[args[k] for k in order]) < 0, (name, bad)
    assert q(1000, 48, 1, 100, 1000, 12, 64) <= q(2000, 48, 1, 100, 2000, 12, 64)


def test_entry_points_reject_null_and_negative_sizes_before_any_launch():
    L = lib()
    E_NULL, E_SIZE, E_RANGE = -1, -2, -6
    rc = L.gae_forest_bin(None, 4, 8, 4, None, 8, None, None, 8, None, None, None)
    assert rc == E_NULL and b"NULL" in L.gae_last_error()
    assert L.gae_forest_bin(None, 4, -1, 4, None, 8, None, None, 8, None, None, None) < 0
    assert b"negative" in L.gae_last_error()
    assert L.gae_forest_bin(None, 3, 8, 4, None, 8, None, None, 8, None, None, None) < 0 and b"ldx" in L.gae_last_error()
    assert L.gae_forest_bin(None, 4, 8, 4, None, 7, None, None, 8, None, None, None) < 0       # rows = NULL, n_rows != n
    assert L.gae_forest_bin(None, 300, 8, 257, None, 8, None, None, 8, None, None, None) < 0
    piv, exp = (ctypes.c_float * 1)(0.0), (ctypes.c_int32 * 1)(0)

    def fit(n_used=8, d=4, bins=8, ldy=1, n=8, t=1, T=2, n_boot=8, depth=3, m=4, msl=1, flags=1, cap=15, ws_bytes=1 << 30,
            pivot=piv, exponent=exp):
        return L.gae_forest_fit(None, None, None, n_used, d, bins, None, ldy, n, t, None, pivot, exponent, T, n_boot, depth, m,
                                msl, flags, 0, None, None, None, None, None, None, None, None, cap, None, None, None, ws_bytes,
                                None)
    assert fit() == E_NULL and b"NULL" in L.gae_last_error()           # everything else is in order: the NULL arrays
    for kw in (dict(n_used=-1), dict(d=0), dict(t=9), dict(T=0), dict(depth=17), dict(bins=1), dict(m=5), dict(m=0),
               dict(msl=0), dict(flags=2), dict(flags=0, n_boot=7, cap=13), dict(ldy=0), dict(n=9), dict(cap=14), dict(n=-1)):
        assert fit(**kw) in (E_SIZE, E_RANGE), kw
    rc = L.gae_forest_predict(None, 4, 8, 4, 1, 2, 15, None, None, None, None, None, None, None, None)
    assert rc == E_NULL and b"NULL" in L.gae_last_error()
    for args in ((None, 4, -1, 4, 1, 2, 15), (None, 3, 8, 4, 1, 2, 15), (None, 4, 8, 0, 1, 2, 15), (None, 4, 8, 4, 9, 2, 15),
                 (None, 4, 8, 4, 1, 0, 15), (None, 4, 8, 4, 1, 2, 0)):
        assert L.gae_forest_predict(*args, None, None, None, None, None, None, None, None) in (E_SIZE, E_RANGE), args


def test_ops_forest_checks_its_options_first():
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import FOREST_KEY_XOR, FOREST_SPLIT_ROWS, GaeHipError
    assert FOREST_KEY_XOR == R.KEY_XOR and FOREST_SPLIT_ROWS == R.SPLIT_ROWS == ops.FOREST_SPLIT_ROWS
    X, y = torch.zeros(10, 4), torch.zeros(10)
    for kw in (dict(n_trees=0), dict(n_trees=1025), dict(n_trees=2.5), dict(max_depth=0), dict(max_depth=17),
               dict(max_bins=1), dict(max_bins=257), dict(min_samples_leaf=0), dict(bootstrap=1), dict(max_features=0),
               dict(max_features=1.5), dict(max_features=0.0), dict(max_features=True), dict(max_samples=0),
               dict(max_samples=2.0), dict(max_samples=5, bootstrap=False), dict(seed=-1), dict(seed=1.0)):
        with pytest.raises(ValueError):
            ops.forest(X, y, **kw)
    with pytest.raises(GaeHipError):                                   # options in order: no CPU fallback
        ops.forest(X, y)
    assert ops.ForestResult._fields[:8] == ("feature", "threshold_bin", "threshold", "left", "count", "value", "gain",
                                            "n_nodes")
