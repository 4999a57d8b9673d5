"""K26 on the device (gae_forest_bin, gae_forest_fit, gae_forest_predict, ops.forest, GAE.forest_graphs, the embed
script) against the numpy restatement tests/forest_ref.py: every tree node for node, every fp64 value bit for bit.

Shapes are the smallest that reach each path: one feature tile and several (d = 37 with t = 3 is two tiles, bins = 256
with t = 8 is three), feature subsets, min_samples_leaf, a bootstrap smaller than the set, no bootstrap, a root just
longer than FOREST_SPLIT_ROWS (cut across blocks, its cells merged by integer atomics), depth 16 on 200 rows (segments
of one sample, the 2 n_boot - 1 capacity), duplicate rows, lossless columns beside continuous ones, a root of four chunks
whose children are longer than a chunk too, over two feature tiles (slots handed out below the root, slot cells of a
second tile).

Targets are multiples of 2^-10 below 2^13, so their fp64 sum is exact in any order and the pivot (the fp64 mean rounded
to fp32) is the same number on the device and in numpy."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import forest_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
S = R.SPLIT_ROWS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    from gae_dgl_amd import ops
    assert ops.FOREST_SPLIT_ROWS == S
    return torch.device("cuda:0")


def as_np(t):
    return t.detach().cpu().numpy()


def grid10(v):
    """rounded to multiples of 2^-10 (exact in fp32 for |v| < 2^13)"""
    return (np.round(np.asarray(v, np.float64) * 1024) / 1024).astype(np.float32)


@functools.lru_cache(maxsize=None)
def data(n, d, t, seed, kind="mixed"):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)).astype(np.float32)
    if kind == "mixed" and d >= 3:
        X[:, 1] = rng.integers(0, 5, n)                                # a lossless column beside continuous ones
        X[:, 2] = np.round(X[:, 2] * 2) / 2                            # a few dozen levels: lossless at 64 bins, not at 8
    if kind == "duplicates":
        X = X[rng.integers(0, n // 4, n)]                              # every row about four times
    w = rng.normal(size=(d, t))
    Y = grid10(X @ w + 2.0 * (X[:, :1] > 0.3) + 0.25 * rng.normal(size=(n, t)))
    return X, (Y[:, 0].copy() if t == 1 else Y)


CASES = {
    "small":        (dict(n=300, d=5, t=1, seed=1), dict(n_trees=3, max_depth=4, max_bins=8, seed=11)),
    "tiles":        (dict(n=1000, d=37, t=3, seed=2), dict(n_trees=4, max_depth=6, max_bins=64, seed=12)),
    "subset":       (dict(n=400, d=10, t=1, seed=3), dict(n_trees=3, max_depth=5, max_bins=32, max_features=3, seed=13)),
    "leaf7":        (dict(n=400, d=6, t=2, seed=4), dict(n_trees=3, max_depth=8, max_bins=32, min_samples_leaf=7, seed=14)),
    "max_samples":  (dict(n=400, d=6, t=1, seed=5), dict(n_trees=3, max_depth=6, max_bins=32, max_samples=150, seed=15)),
    "share":        (dict(n=400, d=6, t=1, seed=5), dict(n_trees=2, max_depth=6, max_bins=32, max_samples=0.3, max_features=0.5,
                                                        seed=25)),
    "no_bootstrap": (dict(n=400, d=6, t=2, seed=6), dict(n_trees=2, max_depth=6, max_bins=32, bootstrap=False, seed=16)),
    "bins256":      (dict(n=700, d=7, t=8, seed=7), dict(n_trees=2, max_depth=5, max_bins=256, seed=17)),
    "long_root":    (dict(n=S + 5, d=3, t=1, seed=8), dict(n_trees=2, max_depth=3, max_bins=16, seed=18)),
    "long_children_tiles": (dict(n=3 * S + 7, d=4, t=8, seed=12), dict(n_trees=2, max_depth=3, max_bins=256, seed=24)),
    "long_plain":   (dict(n=S + 1, d=3, t=2, seed=9), dict(n_trees=1, max_depth=2, max_bins=16, bootstrap=False, seed=19)),
    "depth16":      (dict(n=200, d=4, t=1, seed=10), dict(n_trees=2, max_depth=16, max_bins=64, seed=20)),
    "duplicates":   (dict(n=400, d=5, t=1, seed=11, kind="duplicates"), dict(n_trees=3, max_depth=10, max_bins=64, seed=21)),
    "one_tree":     (dict(n=300, d=5, t=1, seed=1), dict(n_trees=1, max_depth=5, max_bins=16, seed=22)),
    "bins2":        (dict(n=300, d=5, t=1, seed=1), dict(n_trees=2, max_depth=3, max_bins=2, seed=23)),
}


def tile_features(d, bins, words):
    """features per LDS tile: 64 KiB of cells, a u32 count and `words` int64 sums each (csrc/forest_cells.h)"""
    return max(1, min(d, 65536 // (bins * (4 + 8 * words))))


def key_of(name):
    d, kw = CASES[name]
    return tuple(sorted(d.items())), tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def reference(dkey, kwkey, rows=None):
    """the numpy forest of a case, computed once and shared"""
    X, y = data(**dict(dkey))
    return R.forest(X, y, rows=None if rows is None else np.array(rows), **dict(kwkey))


def fit(dev, name, **more):
    from gae_dgl_amd import ops
    d, kw = CASES[name]
    X, y = data(**d)
    return ops.forest(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev), **dict(kw, **more))


INT_FIELDS = ("feature", "threshold_bin", "left", "count", "n_nodes", "n_edges")
BIT_FIELDS = ("threshold", "value", "gain", "edges", "oob_prediction", "oob_rmse", "oob_r2", "importances", "pivot")


def assert_same_forest(res, ref):
    """every field, bit for bit (NaN in the same places)"""
    assert res.n_used == ref.n_used and list(res.exponent) == list(ref.exponent)
    for name in INT_FIELDS + BIT_FIELDS:
        a, b = as_np(getattr(res, name)), np.asarray(getattr(ref, name))
        assert a.shape == b.shape, (name, a.shape, b.shape)
        if name in INT_FIELDS:
            assert a.dtype == np.int32 and np.array_equal(a, b), (name, np.argwhere(a != b)[:5])
        else:
            same = (a.view(np.uint64 if a.dtype == np.float64 else np.uint32) ==
                    b.astype(a.dtype).view(np.uint64 if a.dtype == np.float64 else np.uint32)) | (np.isnan(a) & np.isnan(b))
            assert same.all(), (name, np.argwhere(~same)[:5], a[~same][:3], b[~same][:3])


def same_results(a, b):
    for x, y in zip(a, b):
        if isinstance(x, torch.Tensor):
            if not bool(((x == y) | (x != x) & (y != y)).all()):
                return False
        elif x != y:
            return False
    return True


# ------------------------------------------------------------------ 1. trees equal the reference exactly
@pytest.mark.parametrize("name", sorted(CASES))
def test_forest_equals_the_reference_node_for_node(dev, name):
    res = fit(dev, name)
    ref = reference(*key_of(name))
    assert_same_forest(res, ref)
    T = CASES[name][1]["n_trees"]
    assert res.feature.shape == ref.feature.shape and res.value.shape[0] == T
    if name == "tiles":
        assert int(res.n_nodes.min()) > 30 and res.value.shape[2] == 3
    if name == "depth16":                                              # down to single samples, beyond 2^12 nothing to add
        n_boot = 200
        assert res.feature.shape[1] == 2 * n_boot - 1
        leaves = (as_np(res.feature) < 0) & (as_np(res.count) > 0)
        assert as_np(res.count)[leaves].min() == 1 and int(res.n_nodes.max()) > 150
    if name in ("long_root", "long_plain"):
        assert int(res.count[0, 0]) > S                                # the root was cut across blocks
    if name == "long_children_tiles":                                  # long nodes at level 1, their slots in two tiles
        count, kids = np.asarray(ref.count), np.asarray(ref.left)[:, 0]
        assert (count[:, 0] > S).all() and (count[range(T), kids] > S).all() and (count[range(T), kids + 1] > S).all()
        assert tile_features(4, 256, 8) < 4
    if name == "one_tree":                                             # T = 1: the rows the tree drew have no out-of-bag tree
        oob = as_np(res.oob_prediction)[:, 0]
        drawn = np.zeros(300, bool)
        drawn[ref.samples[0]] = True
        assert np.array_equal(np.isnan(oob), drawn) and 0 < drawn.sum() < 300
    if name == "no_bootstrap":
        assert np.isnan(as_np(res.oob_prediction)).all() and np.isnan(as_np(res.oob_r2)).all()


def test_same_bits_across_runs_streams_strides_and_row_lists(dev):
    from gae_dgl_amd import ops
    X, y = data(n=500, d=6, t=2, seed=30)
    kw = dict(n_trees=3, max_depth=6, max_bins=32, max_features=4, seed=5)
    Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
    first = ops.forest(Xd, yd, **kw)
    assert same_results(first, ops.forest(Xd, yd, **kw))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        other = ops.forest(Xd, yd, **kw)
    stream.synchronize()
    assert same_results(first, other)
    wide = torch.full((500, 11), NAN, device=dev)
    wide[:, 3:9] = Xd
    ywide = torch.full((500, 5), NAN, device=dev)
    ywide[:, 1:3] = yd
    assert same_results(first, ops.forest(wide[:, 3:9], ywide[:, 1:3], **kw))
    # a row list: the other rows hold NaN and are never read; ids and a mask give the same forest as the rows alone
    keep = np.sort(np.random.default_rng(1).choice(500, 320, replace=False))
    alone = ops.forest(Xd[keep], yd[keep], **kw)
    Xh, yh = Xd.clone(), yd.clone()
    mask = torch.zeros(500, dtype=torch.bool, device=dev)
    mask[keep] = True
    Xh[~mask] = NAN
    yh[~mask] = float("inf")
    by_id = ops.forest(Xh, yh, rows=torch.from_numpy(keep).to(dev), **kw)
    by_mask = ops.forest(Xh, yh, rows=mask, **kw)
    assert same_results(alone, by_id) and same_results(alone, by_mask) and by_id.n_used == 320
    assert_same_forest(by_id, R.forest(X, y, rows=keep, **kw))


# ------------------------------------------------------------------ 2. predict
def test_predict_equals_the_reference_and_agrees_with_the_fit(dev):
    from gae_dgl_amd import ops
    X, y = data(**CASES["tiles"][0])
    res, ref = fit(dev, "tiles"), reference(*key_of("tiles"))
    Xd = torch.from_numpy(X).to(dev)
    want = R.predict(ref, X[:300])
    got = as_np(res.predict(Xd[:300]))
    assert got.dtype == np.float64 and got.shape == (300, 3) and np.array_equal(got, want)
    assert np.array_equal(as_np(ops.forest_predict(res, Xd[:1])), want[:1])                    # m = 1
    assert np.array_equal(as_np(res.predict(Xd[:257]))[256], want[256])                        # m = 257: two blocks
    wide = torch.full((300, 40), NAN, device=dev)
    wide[:, 2:39] = Xd[:300]
    assert np.array_equal(as_np(res.predict(wide[:, 2:39])), want)
    # the partition of the fit: without the bootstrap the training rows that reach a leaf are its count
    plain, Xp = fit(dev, "no_bootstrap"), data(**CASES["no_bootstrap"][0])[0]
    tables = R.Forest(*[as_np(v) if isinstance(v, torch.Tensor) else v for v in plain], None, None, None)
    for tree in range(2):
        reached = np.bincount([R.leaf_of(tables, tree, x) for x in Xp], minlength=tables.feature.shape[1])
        leaves = (tables.feature[tree] < 0) & (tables.count[tree] > 0)
        assert np.array_equal(reached[leaves], tables.count[tree][leaves]) and reached[~leaves].sum() == 0


def test_a_row_exactly_on_a_threshold_goes_left(dev):
    res = fit(dev, "one_tree")
    X, _ = data(**CASES["one_tree"][0])
    f, thr, left = int(res.feature[0, 0]), float(res.threshold[0, 0]), int(res.left[0, 0])
    assert f >= 0
    x = np.tile(X[:1], (3, 1))
    x[0, f], x[1, f], x[2, f] = thr, np.nextafter(np.float32(thr), np.float32(np.inf)), np.float32(-1e30)
    tables = R.Forest(*[as_np(v) if isinstance(v, torch.Tensor) else v for v in res], None, None, None)
    got = as_np(res.predict(torch.from_numpy(x).to(dev)))[:, 0]
    nodes = [R.leaf_of(tables, 0, r) for r in x]
    assert got.tolist() == [tables.value[0, k, 0] for k in nodes]
    assert tables.left[0, 0] == left and tables.threshold[0, 0] == np.float32(thr)
    # on the edge and far below it: into the left child's subtree; just above: into the right child's
    under = lambda k, top: k == top or any(under(k, c) for c in ((tables.left[0, top], tables.left[0, top] + 1)
                                                                 if tables.feature[0, top] >= 0 else ()))
    assert under(nodes[0], left) and under(nodes[2], left) and under(nodes[1], left + 1)


def test_a_nan_feature_gives_a_nan_row_and_a_status_count(dev):
    res = fit(dev, "small")
    X, _ = data(**CASES["small"][0])
    x = X[:260].copy()
    x[3, 2], x[200, 0], x[259, 4] = np.nan, np.inf, -np.inf
    status = torch.zeros(4, dtype=torch.int64, device=dev)
    got = as_np(res.predict(torch.from_numpy(x).to(dev), status=status))
    bad = np.zeros(260, bool)
    bad[[3, 200, 259]] = True
    assert np.isnan(got[bad]).all() and not np.isnan(got[~bad]).any()
    assert status.tolist() == [3, 0, 0, 0]
    assert np.array_equal(got[~bad], R.predict(reference(*key_of("small")), x[~bad]))


# ------------------------------------------------------------------ 3. failures
def test_non_finite_listed_rows_raise_and_unlisted_ones_are_never_read(dev):
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    X, y = data(n=300, d=5, t=1, seed=1)
    kw = dict(n_trees=2, max_depth=3, max_bins=8, seed=1)
    for where in ("X", "y"):
        Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
        if where == "X":
            Xd[17, 3] = NAN
        else:
            yd[17] = float("inf")
        with pytest.raises(GaeHipError, match="finite"):
            ops.forest(Xd, yd, **kw)
        rows = torch.tensor([i for i in range(300) if i != 17], device=dev)
        res = ops.forest(Xd, yd, rows=rows, **kw)
        assert_same_forest(res, R.forest(X, y, rows=as_np(rows), **kw))


def test_one_past_each_limit_and_misplaced_targets_are_errors(dev):
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    X = torch.zeros(40, 4, device=dev)
    y = torch.zeros(40, device=dev)
    with pytest.raises(GaeHipError):
        ops.forest(torch.zeros(40, 257, device=dev), y, 2)
    with pytest.raises(GaeHipError):
        ops.forest(X, torch.zeros(40, 9, device=dev), 2)
    for kw in (dict(n_trees=1025), dict(max_depth=17), dict(max_bins=257), dict(max_features=5)):
        with pytest.raises(ValueError):
            ops.forest(X, y, **kw)
    with pytest.raises(GaeHipError):
        ops.forest(X, y.cpu(), 2)
    with pytest.raises(GaeHipError):
        ops.forest(X, torch.zeros(39, device=dev), 2)
    with pytest.raises(GaeHipError):
        ops.forest(X, y.long(), 2)
    with pytest.raises(GaeHipError):
        ops.forest(X, y, 2, rows=torch.tensor([0, 40], device=dev))
    with pytest.raises(GaeHipError):
        ops.forest(X, y, 2, rows=torch.zeros(40, dtype=torch.bool, device=dev))
    res = ops.forest(X, y, 2)                                          # constant everything: one node per tree
    assert res.n_nodes.tolist() == [1, 1] and float(res.value.abs().max()) == 0.0
    with pytest.raises(GaeHipError):
        res.predict(torch.zeros(3, 5, device=dev))


# ------------------------------------------------------------------ 4. the method, not only the port
def test_a_step_and_a_slope_are_found_and_credited(dev):
    """y = 2 [x3 > 0.25] - x7: the out-of-bag R2 is the reference's own, and features 3 and 7 carry more importance than
    all the others together (the CPU reference gives 0.9997 of it to them)"""
    from gae_dgl_amd import ops
    rng = np.random.default_rng(42)
    X = rng.uniform(-1, 1, size=(2000, 10)).astype(np.float32)
    y = grid10(2.0 * (X[:, 3] > 0.25) - X[:, 7])
    kw = dict(n_trees=16, max_depth=6, seed=7)
    res = ops.forest(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev), **kw)
    ref = R.forest(X, y, **kw)
    assert float(res.oob_r2[0]) == ref.oob_r2[0] and ref.oob_r2[0] > 0.9
    imp = as_np(res.importances)
    assert np.array_equal(imp, ref.importances)
    assert imp[3] + imp[7] > imp.sum() - imp[3] - imp[7]


# ------------------------------------------------------------------ 5. the surface
def test_forest_graphs_is_forest_of_the_molecule_features(dev):
    import gae_dgl_amd as G
    from gae_dgl_amd import ops
    from gae_dgl_amd.dataset import DeviceGraphDataset
    data_ = DeviceGraphDataset.synthetic_zinc(300, seed=1, device=dev)
    torch.manual_seed(0)
    model = G.GAE(39, [32, 16]).to(dev).eval()
    y = torch.randn(300, 2, generator=torch.Generator().manual_seed(2)).to(dev)
    feats = model.embed_graphs(data_)
    kw = dict(n_trees=4, max_depth=5, max_features=16, seed=3)
    want = ops.forest(feats, y, **kw)
    res = model.forest_graphs(data_, y, fused="auto", batch_size=256, **kw)
    assert same_results(res, want) and res.n_used == 300 and res.edges.shape == (48, 63)
    with pytest.raises(ValueError):
        model.forest_graphs(data_, y, grad=True)


def test_cli_embed_forest_in_a_child_process(tmp_path):
    import gae_dgl_amd as G
    torch.manual_seed(0)
    ckpt = str(tmp_path / "m.pkl")
    torch.save(G.GAE(39, [32, 16]).state_dict(), ckpt)
    ng = 200
    np.save(tmp_path / "y.npy", np.random.default_rng(1).standard_normal((ng, 2)))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "gae_dgl_amd.embed", "--checkpoint", ckpt, "--hidden_dims", "32", "16",
                        "--synthetic", str(ng), "--out", str(tmp_path / "f.npy"), "--targets", str(tmp_path / "y.npy"),
                        "--forest", "8", "--forest_depth", "5", "--forest_features", "16", "--forest_out",
                        str(tmp_path / "model.npz"), "--ridge", "1.0", "--ridge_folds", "3"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("Random Forest (8 trees, depth 5, out-of-bag) ")]
    assert len(line) == 1 and line[0].count("RMSE:") == 2 and line[0].count("R2:") == 2, r.stdout
    assert f"Grew a forest on {ng} molecules, 8 trees" in r.stdout and "Ridge (3-fold CV" in r.stdout
    z = np.load(tmp_path / "model.npz")
    assert z["feature"].shape == (8, 63) and z["value"].shape == (8, 63, 2) and z["importances"].shape == (48,)
    nums = [float(v) for v in line[0].split(") ")[1].replace("RMSE: ", "").replace("R2: ", "").split(" | ")]
    assert nums == pytest.approx([z["oob_rmse"][0], z["oob_r2"][0], z["oob_rmse"][1], z["oob_r2"][1]], abs=2e-6)
