"""K34 on the device (gae_tanimoto_knn, ops.tanimoto_knn, the gae_dgl_amd.fingerprint script): index and value bit for bit
against the numpy restatement tests/fingerprint_ref.py.  Shapes are the smallest at which each mechanism can break: one
lane and wave tails (m = 1, 31, 33, 65), more than one block of 256 queries (m = 257), tile tails of the 16-row tile
(n = 1 .. 65, 130), several tiles per split and several splits (n = 2708), every register form of the query
(W = 1, 2, 3 -> 4, 32, 64), k = 1, k > n and the largest k."""
import numpy as np
import pytest
import torch

import fingerprint_ref as R

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def as_np(t):
    return t.detach().cpu().numpy()


def strided(X, pad, dev):
    """X [n, W] on the device as a view of a [n, W + pad] buffer whose pad words are all ones: never read as data"""
    X = torch.as_tensor(X, dtype=torch.int32)
    buf = torch.full((X.shape[0], X.shape[1] + pad), -1, dtype=torch.int32)
    buf[:, :X.shape[1]] = X
    return buf.to(dev)[:, :X.shape[1]]


def raw_tanimoto(Q, X, k, flags=0, splits=0, pad=3):
    """gae_tanimoto_knn on device tensors (strided views allowed) into outputs with ldo = k + pad; the pad columns are
    checked to be untouched.  Returns (index int32 [m, k], value fp32 [m, k]) on the host"""
    from gae_dgl_amd import _lib
    from gae_dgl_amd.ops import _ptr, _stream
    m, W = Q.shape
    n = X.shape[0]
    ldq = Q.stride(0) if m > 1 else W
    ldx = X.stride(0) if n > 1 else W
    nbytes = _lib.load().gae_tanimoto_knn_workspace_bytes(m, n, W, k, splits)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=Q.device)
    index = torch.full((m, k + pad), -7, dtype=torch.int32, device=Q.device)
    value = torch.full((m, k + pad), NAN, dtype=torch.float32, device=Q.device)
    _lib.call("gae_tanimoto_knn", _ptr(Q), ldq, m, _ptr(X), ldx, n, W, k, flags, splits, _ptr(index), _ptr(value), k + pad,
              _ptr(ws), ws.numel(), _stream())
    torch.cuda.synchronize()
    assert bool((index[:, k:] == -7).all()) and bool(torch.isnan(value[:, k:]).all()), "a store beyond k"
    return as_np(index[:, :k]), as_np(value[:, :k])


def bit_rows(rng, n, W, lo=0.01, hi=0.5):
    """int32 [n, W]: random bit rows, every row with its own density in [lo, hi]"""
    p = rng.uniform(lo, hi, (n, 1))
    return R.pack_bits(rng.random((n, 32 * W)) < p)


def same_bits(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int32), want[1].view(np.int32))


# ------------------------------------------------------------------ 1. bit for bit on a covering set of shapes
MS, NS, WS, KS = [1, 31, 33, 65, 257], [1, 2, 63, 64, 65, 130, 2708], [1, 2, 3, 32, 64], [1, 5, 64]
CASES = sorted({(MS[i % 5], NS[i % 7], WS[(i // 2) % 5], KS[(i // 3) % 3]) for i in range(35)}
               | {(257, 2708, 64, 64), (65, 2708, 32, 64), (257, 130, 3, 5), (33, 2708, 1, 64)})


def test_the_cases_cover_every_value_of_every_axis():
    for axis, values in enumerate((MS, NS, WS, KS)):
        assert set(values) <= {c[axis] for c in CASES}


@pytest.mark.parametrize("m, n, W, k", CASES)
def test_exact_on_random_rows_with_ties_and_empty_rows(dev, m, n, W, k):
    """densities 1 % - 50 %; empty rows on both sides (u = 0: value 0.0); blocks of identical database rows, so most of a
    top-k is ties and the index rule decides; the queries themselves are in X (value 1.0)"""
    rng = np.random.default_rng(m * 1000003 + n * 1009 + W * 17 + k)
    Q, X = bit_rows(rng, m, W), bit_rows(rng, n, W)
    Q[::7] = 0
    X[::5] = 0
    if n >= 63:
        X[8:40] = X[8]                                                 # 32 identical rows across two tiles
        X[n - 20:] = X[n - 20]
        take = rng.integers(0, m, 6)
        X[40:46] = Q[take]                                             # queries present in the database
    want = R.tanimoto_knn(Q, X, k)
    Qd, Xd = strided(Q, 5, dev), strided(X, 2, dev)
    for splits in (0, 2):
        got = raw_tanimoto(Qd, Xd, k, splits=splits)
        assert np.array_equal(got[0], want[0]), (splits, np.argwhere(got[0] != want[0])[:4])
        assert same_bits(got, want), splits
    if n >= 63 and k >= 5:
        V = R.tanimoto_matrix(Q[take], X)
        assert (V.max(1)[Q[take].any(1)] == 1.0).all()
    if k > n:
        assert (want[0][:, n:] == -1).all() and (want[1][:, n:] == -INF).all()


def test_empty_database_and_empty_query_set(dev):
    Q = torch.from_numpy(bit_rows(np.random.default_rng(0), 5, 4)).to(dev)
    i, v = raw_tanimoto(Q, torch.empty(0, 4, dtype=torch.int32, device=dev), 3)
    assert (i == -1).all() and (v == -INF).all()
    i, v = raw_tanimoto(torch.empty(0, 4, dtype=torch.int32, device=dev), Q, 3)
    assert i.shape == (0, 3)


@pytest.mark.parametrize("n, W, k", [(65, 3, 5), (300, 1, 64), (2708, 32, 5)])
def test_self_search_leaves_the_row_out(dev, n, W, k):
    rng = np.random.default_rng(n + W)
    X = bit_rows(rng, n, W)
    X[n // 2:] = X[:n - n // 2]                                        # every row of the first half has a twin
    X[3] = 0
    want = R.tanimoto_knn(X, X, k, exclude_same=True)
    got = raw_tanimoto(strided(X, 1, dev), strided(X, 1, dev), k, flags=1)
    assert same_bits(got, want)
    assert not (got[0] == np.arange(n)[:, None]).any()
    from gae_dgl_amd import ops
    res = ops.tanimoto_knn(torch.from_numpy(X).to(dev), k=k)
    assert same_bits((as_np(res.index), as_np(res.value)), want)


def test_same_bits_for_any_split_stride_and_run(dev):
    from gae_dgl_amd import ops
    rng = np.random.default_rng(5)
    Q, X = bit_rows(rng, 300, 8), bit_rows(rng, 5000, 8)
    X[1000:1100] = X[1000]
    Qd, Xd = torch.from_numpy(Q).to(dev), torch.from_numpy(X).to(dev)
    base = ops.tanimoto_knn(Qd, Xd, k=7)
    assert same_bits((as_np(base.index), as_np(base.value)), R.tanimoto_knn(Q, X, 7))
    runs = [ops.tanimoto_knn(Qd, Xd, k=7, splits=s) for s in (1, 3, 16)]
    runs.append(ops.tanimoto_knn(strided(Q, 11, dev), strided(X, 4, dev), k=7))
    runs.append(ops.tanimoto_knn(Qd.t().contiguous().t(), Xd, k=7, splits=5))      # inner stride != 1: copied
    runs.append(ops.tanimoto_knn(Qd, Xd, k=7))
    for r in runs:
        assert torch.equal(r.index, base.index)
        assert torch.equal(r.value.view(torch.int32), base.value.view(torch.int32))
    self0 = ops.tanimoto_knn(Xd, k=64)
    for s in (1, 3, 16):
        r = ops.tanimoto_knn(Xd, k=64, splits=s)
        assert torch.equal(r.index, self0.index) and torch.equal(r.value, self0.value)


@pytest.mark.parametrize("k", [5, 64])
@pytest.mark.parametrize("n", [1, 17, 33])
def test_more_splits_than_tiles(dev, n, k):
    """16 column splits over a database of one to three tiles of 16 rows: the parts are whole tiles, so all but one to
    three of them are empty (pb = pe = n) and their blocks write lists of padding alone; at k = 64 no query has k
    candidates.  Every call must give the reference's bits, and so the bits of one split"""
    rng = np.random.default_rng(n * 100 + k)
    m, W = 33, 3
    Q, X = bit_rows(rng, m, W), bit_rows(rng, n, W)
    X[::4] = X[0]                                                      # ties: the index rule decides across the parts
    searches = [(Q, X, 0)] + ([(X, X, 1)] if n == m else [])           # (queries, database, same-index flag)
    for A, B, flag in searches:
        Ad, Bd = strided(A, 5, dev), strided(B, 2, dev)
        want = R.tanimoto_knn(A, B, k, exclude_same=bool(flag))
        one = raw_tanimoto(Ad, Bd, k, flags=flag, splits=1)
        many = raw_tanimoto(Ad, Bd, k, flags=flag, splits=16)
        assert same_bits(one, want) and same_bits(many, want) and same_bits(one, many), flag
        assert (want[0][:, min(n - flag, k):] == -1).all() and (want[0][:, :min(n - flag, k)] >= 0).all()


def test_no_fallback_and_argument_errors(dev):
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    X = torch.zeros(40, 4, dtype=torch.int32, device=dev)
    for bad in (dict(k=0), dict(k=65)):
        with pytest.raises(GaeHipError):
            ops.tanimoto_knn(X, **bad)
    with pytest.raises(GaeHipError):
        ops.tanimoto_knn(torch.zeros(40, 65, dtype=torch.int32, device=dev), k=3)
    with pytest.raises(GaeHipError):
        ops.tanimoto_knn(X, torch.zeros(40, 5, dtype=torch.int32, device=dev), k=3)
    with pytest.raises(GaeHipError):
        ops.tanimoto_knn(X.long(), k=3)


# ------------------------------------------------------------------ 2. real fingerprints, end to end
@pytest.fixture(scope="module")
def zinc300():
    from gae_dgl_amd import workloads
    gp, src, dst, X = workloads.zinc_like(300, 0)
    ip, ix = R.csr_of(int(gp[-1]), src, dst)
    return R.fingerprint_bits(gp, ip, ix, X, 2, 1024), R.fingerprint_counts(gp, ip, ix, X, 2, 1024)


def test_self_search_of_real_fingerprints(dev, zinc300):
    from gae_dgl_amd import ops
    from gae_dgl_amd.dataset import DeviceGraphDataset
    words, _ = zinc300
    data = DeviceGraphDataset.synthetic_zinc(300, seed=0, device=dev)
    fp = data.fingerprints()
    assert np.array_equal(as_np(fp), words)
    for k in (10, 64):
        res = ops.tanimoto_knn(fp, k=k)
        assert same_bits((as_np(res.index), as_np(res.value)), R.tanimoto_knn(words, words, k, exclude_same=True))
    hit = ops.tanimoto_knn(fp[[7, 299]], fp, k=1)
    assert as_np(hit.index)[:, 0].tolist() == [7, 299] and as_np(hit.value)[:, 0].tolist() == [1.0, 1.0]


def test_the_script_in_process(dev, zinc300, tmp_path, capsys):
    from gae_dgl_amd import fingerprint as F
    from gae_dgl_amd import ops
    words, counts = zinc300
    ng, k = 300, 5
    y = np.random.default_rng(1).standard_normal(ng)
    np.save(tmp_path / "y.npy", y)
    out = F.main(["--synthetic", str(ng), "--out", str(tmp_path / "fp.npy"), "--neighbours", str(k), "--neighbours_out",
                  str(tmp_path / "nn.npz"), "--targets", str(tmp_path / "y.npy"), "--ridge", "--forest", "10"])
    text = capsys.readouterr().out
    saved = np.load(tmp_path / "fp.npy")
    assert saved.dtype == np.int32 and np.array_equal(saved, words) and np.array_equal(out, words)
    z = np.load(tmp_path / "nn.npz")
    want = R.tanimoto_knn(words, words, k, exclude_same=True)
    assert z["index"].dtype == np.int32 and z["value"].dtype == np.float32 and same_bits((z["index"], z["value"]), want)
    assert torch.equal(F.main.neighbours.index.cpu(), torch.from_numpy(want[0]))
    head = f"ECFP-like (r = 2, 1024 bits) kNN ({k}, Tanimoto, leave-one-out) RMSE:"
    line = [l for l in text.splitlines() if l.startswith(head)]
    assert len(line) == 1, text
    err = y[z["index"]].mean(1) - y
    stats = {"RMSE": np.sqrt((err ** 2).mean()), "MAE": np.abs(err).mean(),
             "R2": 1 - (err ** 2).sum() / ((y - y.mean()) ** 2).sum()}
    fields = dict(f.split(":") for f in line[0].split("leave-one-out) ")[1].split(" | "))
    for key, v in stats.items():
        assert float(fields[key]) == pytest.approx(v, abs=2e-6)
    # the heads ran on the count fingerprint folded to their width limits, with their defaults
    dev_counts = torch.from_numpy(counts).to(dev)
    yd = torch.from_numpy(y.astype(np.float32)).to(dev)
    ridge = [l for l in text.splitlines() if l.startswith("ECFP-like (r = 2, 128 counts) Ridge (5-fold CV, lambda = ")]
    forest = [l for l in text.splitlines()
              if l.startswith("ECFP-like (r = 2, 256 counts) Random Forest (10 trees, depth 12, out-of-bag) RMSE: ")]
    assert len(ridge) == 1 and len(forest) == 1, text
    r = ops.ridge(ops.fingerprint_fold(dev_counts, 128).float(), yd, None, folds=5, seed=0)
    assert F.main.ridge.lam == r.lam and torch.equal(F.main.ridge.coef, r.coef)
    chosen = r.lambdas.tolist().index(r.lam)
    assert float(ridge[0].split("RMSE: ")[1].split(" |")[0]) == pytest.approx(float(r.cv_rmse[chosen, 0]), abs=2e-6)
    f = ops.forest(ops.fingerprint_fold(dev_counts, 256).float(), yd, 10, seed=0)
    assert torch.equal(F.main.forest.feature, f.feature) and torch.equal(F.main.forest.threshold_bin, f.threshold_bin)
    assert torch.equal(F.main.forest.oob_prediction.nan_to_num(nan=-99.0),      # (NaN: a row no tree left out of its bag)
                       f.oob_prediction.nan_to_num(nan=-99.0))
    assert float(forest[0].split("RMSE: ")[1].split(" |")[0]) == pytest.approx(float(f.oob_rmse[0]), abs=2e-6)
    assert float(forest[0].split("R2: ")[1]) == pytest.approx(float(f.oob_r2[0]), abs=2e-6)
