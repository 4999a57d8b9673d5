"""K24 without a GPU: the argument errors of gae_knn (returned before anything is dereferenced), its workspace query, the
fp64 restatement tests/knn_ref.py against hand-worked cases, metrics.knn_predict / regression_metrics against
hand-computed values, and the argument errors of the two command lines."""
import math

import numpy as np
import pytest
import torch

import knn_ref as R

E_NULL, E_SIZE, E_WORKSPACE, E_RANGE = -1, -2, -5, -6
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    return _lib.load()


def call(lib, *, ldq=8, m=4, ldx=8, n=10, d=8, k=3, metric=0, flags=0, splits=0, index=1 << 20, value=1 << 21, ldo=3,
         ws=1 << 22, ws_bytes=1 << 30, Q=1 << 23, X=1 << 24):
    """gae_knn with made-up non-NULL addresses: an argument error must return before any of them is touched"""
    rc = lib.gae_knn(Q, ldq, m, X, ldx, n, d, k, metric, flags, splits, index, value, ldo, ws, ws_bytes, None)
    return rc, lib.gae_last_error().decode()


@pytest.mark.parametrize("kw, code, text", [
    (dict(d=0), E_RANGE, "d = 0 outside 1..256"),
    (dict(d=257, ldq=300, ldx=300), E_RANGE, "d = 257 outside 1..256"),
    (dict(k=0), E_RANGE, "k = 0 outside 1..64"),
    (dict(k=65, ldo=65), E_RANGE, "k = 65 outside 1..64"),
    (dict(m=-1), E_SIZE, "negative m = -1"),
    (dict(n=-1), E_SIZE, "negative m = 4 or n = -1"),
    (dict(m=1 << 31), E_SIZE, "beyond int32 indices"),
    (dict(n=1 << 31), E_SIZE, "beyond int32 indices"),
    (dict(ldq=7), E_SIZE, "leading dimension too small (ldq 7 < d"),
    (dict(ldx=7), E_SIZE, "ldx 7 < d"),
    (dict(ldo=2), E_SIZE, "ldo 2 < k"),
    (dict(metric=2), E_RANGE, "unknown metric 2"),
    (dict(metric=-1), E_RANGE, "unknown metric -1"),
    (dict(flags=2), E_RANGE, "unknown flags 0x2"),
    (dict(splits=17), E_RANGE, "splits = 17 outside 0..16"),
    (dict(splits=-1), E_RANGE, "splits = -1 outside 0..16"),
    (dict(index=None), E_NULL, "index_out / value_out is NULL"),
    (dict(value=None), E_NULL, "index_out / value_out is NULL"),
    (dict(Q=None), E_NULL, "Q is NULL"),
    (dict(X=None), E_NULL, "X is NULL"),
    (dict(ws=None), E_NULL, "workspace is NULL"),
    (dict(ws_bytes=16), E_WORKSPACE, "workspace of 16 bytes"),
    # two bad arguments: the one that is checked first is the one reported
    (dict(d=257, ldq=300, ldx=300, k=65, ldo=65), E_RANGE, "d = 257 outside 1..256"),
    (dict(metric=2, flags=2), E_RANGE, "unknown metric 2"),
])
def test_argument_errors_come_before_any_access(lib, kw, code, text):
    rc, msg = call(lib, **kw)
    assert rc == code, (rc, msg)
    assert msg.startswith("gae_knn: ") and text in msg, msg


def test_empty_query_set_is_not_an_error(lib):
    assert call(lib, m=0, index=None, value=None, Q=None, X=None)[0] == 0


def test_workspace_query_is_a_monotone_host_function(lib):
    q = lib.gae_knn_workspace_bytes
    assert q(0, 0, 1, 1, 0) > 0 and q(100, 1000, 48, 10, 0) == q(100, 1000, 48, 10, 0)
    for splits in (0, 1, 3, 16):
        prev = 0
        for m in (0, 1, 31, 32, 33, 127, 128, 129, 4096, 34944, 35072, 249455, 10 ** 6, 2 ** 31 - 1):
            cur = q(m, 249455, 48, 10, splits)
            assert cur >= prev > -1, (m, splits)
            prev = cur
        prev = 0
        for n in (0, 1, 255, 256, 257, 4096, 249455, 2 ** 31 - 1):
            cur = q(4096, n, 48, 10, splits)
            assert cur >= prev > -1, (n, splits)
            prev = cur
        prev = 0
        for k in range(1, 65):
            cur = q(4096, 249455, 48, k, splits)
            assert cur >= prev > -1, (k, splits)
            prev = cur
    prev = 0
    for splits in range(1, 17):
        cur = q(4096, 249455, 48, 10, splits)
        assert cur > prev
        prev = cur
    # never the m x n matrix: linear in n + m k splits
    assert q(249455, 249455, 48, 10, 0) < 4 * 249455 + 8 * 10 * 16 * 249455 + 4096
    assert q(10, 10, 0, 1, 0) == E_RANGE and q(10, 10, 8, 65, 0) == E_RANGE and q(-1, 10, 8, 1, 0) == E_SIZE
    assert q(10, 10, 8, 1, 17) == E_RANGE and b"splits = 17" in lib.gae_last_error()


# ------------------------------------------------------------------ the reference against hand-worked cases
def test_reference_on_a_hand_worked_case_with_ties_and_padding():
    Q = np.array([[0.0], [1.0]])
    X = np.array([[1.0], [-1.0], [1.0], [3.0]])
    idx, val = R.knn(Q, X, 3, "l2")
    assert idx.dtype == np.int32
    assert idx.tolist() == [[0, 1, 2], [0, 2, 1]]                      # query 0: three rows at distance 1, lowest j first
    assert val.tolist() == [[1.0, 1.0, 1.0], [0.0, 0.0, 4.0]]
    idx, val = R.knn(Q, X, 5, "l2")                                    # k > n: padding
    assert idx.tolist() == [[0, 1, 2, 3, -1], [0, 2, 1, 3, -1]]
    assert val.tolist() == [[1.0, 1.0, 1.0, 9.0, INF], [0.0, 0.0, 4.0, 4.0, INF]]
    idx, val = R.knn(Q, X, 3, "dot")
    assert idx.tolist() == [[0, 1, 2], [3, 0, 2]]                      # query 0: every product is 0
    assert val.tolist() == [[0.0, 0.0, 0.0], [3.0, 1.0, 1.0]]
    # a self-search: the row itself is absent, its duplicate is a neighbour at distance exactly 0
    idx, val = R.knn(X, X, 3, "l2", exclude_same=True)
    assert idx.tolist() == [[2, 1, 3], [0, 2, 3], [0, 1, 3], [0, 2, 1]]
    assert val.tolist() == [[0.0, 4.0, 4.0], [4.0, 4.0, 16.0], [0.0, 4.0, 4.0], [4.0, 4.0, 16.0]]
    idx, val = R.knn(X, X, 4, "dot", exclude_same=True)
    assert idx[3].tolist() == [0, 2, 1, -1] and val[3].tolist() == [3.0, 3.0, -3.0, -INF]


def test_reference_leaves_out_rows_without_a_finite_key():
    Q = np.array([[0.0, 0.0], [np.nan, 0.0], [1.0, 1.0]])
    X = np.array([[1.0, 0.0], [np.inf, 0.0], [0.0, np.nan], [2.0, 2.0]])
    idx, val = R.knn(Q, X, 3, "l2")
    assert idx.tolist() == [[0, 3, -1], [-1, -1, -1], [0, 3, -1]]
    assert val[0].tolist() == [1.0, 8.0, INF] and val[2].tolist() == [1.0, 2.0, INF]
    idx, val = R.knn(Q, X, 2, "dot")
    assert idx.tolist() == [[0, 3], [-1, -1], [3, 0]] and val[1].tolist() == [-INF, -INF]
    assert R.knn(Q, np.zeros((0, 2)), 2, "l2")[0].tolist() == [[-1, -1]] * 3


def test_tolerant_check_accepts_the_exact_answer_and_names_a_wrong_one():
    rng = np.random.default_rng(0)
    Q, X = rng.standard_normal((40, 5)), rng.standard_normal((300, 5))
    idx, val = R.knn(Q, X, 7, "l2")
    assert R.check_tolerant(Q, X, idx, val) == []
    wrong = idx.copy(); wrong[3, 6] = int(np.argmax(((Q[3] - X) ** 2).sum(1)))      # the farthest row
    assert any("row 3" in s for s in R.check_tolerant(Q, X, wrong, R.pair_values(Q, X, wrong, "l2")))
    rep = idx.copy(); rep[5, 1] = rep[5, 0]
    assert R.check_tolerant(Q, X, rep, val) != []
    unsorted = val.copy(); unsorted[0, :2] = unsorted[0, 1::-1] + np.array([1e-3, 0])
    assert any("ascending" in s for s in R.check_tolerant(Q, X, idx, unsorted))


def test_a_reported_expanded_form_would_fail_the_direct_distance_bound():
    """the data of the GPU test 'the reported distance is the direct one': features with a common offset of +20.  The
    expanded form |q|^2 - 2 q.x + |x|^2 in fp32 misses the bound the direct chain keeps"""
    rng = np.random.default_rng(4)
    d = 48
    Q = (rng.standard_normal((200, d)) + 20).astype(np.float32)
    X = (rng.standard_normal((1000, d)) + 20).astype(np.float32)
    idx, D = R.knn(Q, X, 10, "l2")
    bound = 2 * (d + 2) * 2.0 ** -24 * D + 1e-30
    direct = ((Q[:, None, :] - X[idx]) ** 2).sum(-1, dtype=np.float32)               # fp32, taken directly
    assert (np.abs(direct.astype(np.float64) - D) <= bound).all()
    expanded = R.expanded_fp32(Q, X, idx)
    assert (np.abs(expanded.astype(np.float64) - D) > bound).mean() > 0.5


# ------------------------------------------------------------------ metrics
def test_knn_predict_regression_by_hand():
    from gae_dgl_amd import metrics
    y = torch.tensor([1.0, 3.0, 5.0, float("nan")])
    index = torch.tensor([[0, 1, -1], [2, -1, -1], [-1, -1, -1], [0, 3, 2]], dtype=torch.int32)
    value = torch.tensor([[1.0, 4.0, INF], [0.0, INF, INF], [INF, INF, INF], [4.0, 9.0, 16.0]])
    p = metrics.knn_predict(index, value, y)
    assert p.dtype == torch.float64 and p[:2].tolist() == [2.0, 5.0] and math.isnan(float(p[2]))
    assert float(p[3]) == 3.0                                           # the NaN target does not vote: (1 + 5) / 2
    w = metrics.knn_predict(index, value, y, weights="distance")
    # row 0: weights 1 / 1 and 1 / 2 -> (1 + 1.5) / 1.5; row 3: 1 / 2 and 1 / 4 -> (0.5 + 1.25) / 0.75
    assert float(w[0]) == pytest.approx(5.0 / 3.0, rel=1e-9) and float(w[3]) == pytest.approx(7.0 / 3.0, rel=1e-9)
    assert float(w[1]) == pytest.approx(5.0, rel=1e-9)                  # distance 0: one voter, its own target
    assert math.isnan(float(w[2]))
    with pytest.raises(ValueError):
        metrics.knn_predict(index, value, y, task="ranking")
    with pytest.raises(ValueError):
        metrics.knn_predict(index, value, y, weights="rank")
    with pytest.raises(ValueError):
        metrics.knn_predict(index, value[:, :2], y)
    with pytest.raises(ValueError):
        metrics.knn_predict(torch.tensor([[7]]), torch.tensor([[1.0]]), y)


def test_knn_predict_classification_by_hand():
    from gae_dgl_amd import metrics
    y = torch.tensor([2, 0, 0, -1, 1, 1])
    index = torch.tensor([[1, 2, 0],        # classes 0, 0, 2 -> 0
                          [0, 4, 1],        # 2, 1, 0: a three-way tie -> the lower class 0
                          [4, 5, 0],        # 1, 1, 2 -> 1
                          [3, 0, -1],       # unlabelled, 2, padding -> 2
                          [3, -1, -1],      # the only neighbour is unlabelled -> no voter
                          [-1, -1, -1]])    # all padding -> no voter
    value = torch.tensor([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [4.0, 4.0, 0.25], [1.0, 1.0, INF], [1.0, INF, INF],
                          [INF, INF, INF]])
    p = metrics.knn_predict(index, value, y, task="classification")
    assert p.dtype == torch.int64 and p.tolist() == [0, 0, 1, 2, -1, -1]
    # distance weights: row 2 has 1/2 + 1/2 for class 1 against 1 / 0.5 = 2 for class 2 -> 2
    pw = metrics.knn_predict(index, value, y, task="classification", weights="distance", n_classes=4)
    assert pw.tolist() == [0, 0, 2, 2, -1, -1]
    with pytest.raises(ValueError):
        metrics.knn_predict(index, value, y, task="classification", n_classes=2)
    with pytest.raises(ValueError):
        metrics.knn_predict(index, value, y.float(), task="classification")


def test_regression_metrics_by_hand():
    from gae_dgl_amd import metrics
    r = metrics.regression_metrics(torch.tensor([1.0, 2.0, 4.0, float("nan")]), torch.tensor([1.0, 3.0, 2.0, 9.0]))
    # errors 0, -1, 2 over targets 1, 3, 2 (mean 2, SST 2): SSE 5
    assert r["n"] == 3 and r["left_out"] == 1
    assert r["rmse"] == pytest.approx(math.sqrt(5.0 / 3.0)) and r["mae"] == pytest.approx(1.0)
    assert r["r2"] == pytest.approx(1.0 - 5.0 / 2.0)
    perfect = metrics.regression_metrics([1.0, 2.0], [1.0, 2.0])
    assert perfect["rmse"] == 0.0 and perfect["r2"] == 1.0
    none = metrics.regression_metrics([float("nan")], [1.0])
    assert none["n"] == 0 and math.isnan(none["rmse"])
    assert math.isnan(metrics.regression_metrics([1.0, 2.0], [3.0, 3.0])["r2"])
    with pytest.raises(ValueError):
        metrics.regression_metrics([1.0], [1.0, 2.0])


# ------------------------------------------------------------------ the wrapper and the command lines
def test_ops_knn_has_no_cpu_fallback_and_checks_its_options():
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    X = torch.randn(10, 4)
    with pytest.raises(GaeHipError):
        ops.knn(X, k=3)                                                # a CPU tensor
    with pytest.raises(ValueError):
        ops.knn(X, k=3, metric="manhattan")
    with pytest.raises(ValueError):
        ops.knn(X, X, k=3, exclude_self=True)
    with pytest.raises(ValueError):
        ops.knn(X, k=3, splits=17)
    with pytest.raises(ValueError):
        ops.knn(X)
    assert ops.KNNResult._fields == ("index", "value")


@pytest.mark.parametrize("argv, text", [
    (["--neighbours", "0"], "K must lie in 1..64"),
    (["--neighbours", "65"], "K must lie in 1..64"),
    (["--metric", "dot"], "need --neighbours K"),
    (["--neighbours_out", "nn.npz"], "need --neighbours K"),
    (["--targets", "y.npy"], "need --neighbours K"),
    (["--neighbours", "5", "--targets", "/no/such/file.npy"], "no such file"),
    (["--neighbours", "5", "--metric", "manhattan"], "invalid choice"),
])
def test_embed_argument_errors(argv, text, capsys):
    from gae_dgl_amd import embed as E
    base = ["--checkpoint", "c.pkl", "--hidden_dims", "32", "16", "--synthetic", "10", "--out", "f.npy"]
    with pytest.raises(SystemExit):
        E.parse_args(base + argv)
    assert text in capsys.readouterr().err
    ok = E.parse_args(base + ["--neighbours", "5", "--metric", "cosine", "--neighbours_out", "nn.npz"])
    assert ok.neighbours == 5 and ok.metric == "cosine"


def test_embed_refuses_features_wider_than_the_kernel(capsys):
    from gae_dgl_amd import embed as E
    with pytest.raises(SystemExit):
        E.parse_args(["--checkpoint", "c.pkl", "--hidden_dims", "32", "86", "--synthetic", "10", "--out", "f.npy",
                      "--fused", "off", "--neighbours", "5"])
    assert "3 d = 258 must not exceed 256" in capsys.readouterr().err


@pytest.mark.parametrize("argv, text", [
    (["--knn", "0"], "K must lie in 1..64"),
    (["--knn", "65"], "K must lie in 1..64"),
    (["--knn_metric", "dot"], "--knn_metric needs --knn K"),
    (["--knn", "5", "--knn_metric", "manhattan"], "invalid choice"),
])
def test_train_transductive_argument_errors(argv, text, capsys):
    from gae_dgl_amd import train_transductive as TT
    with pytest.raises(SystemExit):
        TT.parse_args(["--dataset", "cora"] + argv)
    assert text in capsys.readouterr().err
    assert TT.parse_args(["--dataset", "cora", "--knn", "5", "--knn_metric", "cosine"]).knn == 5
