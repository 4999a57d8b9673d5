"""CPU-side checks of K23 (gae_kmeans_*): the ABI and its argument errors without a GPU, the clustering scores, the
class labels of the citation data, and the fp64 restatement tests/kmeans_ref.py against itself."""
import argparse
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

import kmeans_ref as R
from sampled_ref import philox4x32_10
from test_dataset_cpu import _write_planetoid

GAE_E_SIZE, GAE_E_RANGE = -2, -6
SYMBOLS = ["gae_kmeans_workspace_bytes", "gae_kmeans_assign", "gae_kmeans_step", "gae_kmeans_init_pp"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    return _lib.load()


def test_symbols_are_exported_and_bound(lib):
    from gae_dgl_amd import _lib
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "gae_hip_experimental.h")).read()
    core = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gae_hip.h")).read()
    for s in SYMBOLS:
        assert s + "(" in header and s not in core


def test_argument_errors_do_not_need_a_gpu(lib):
    X = (ctypes.c_float * 64)()
    out = (ctypes.c_int32 * 64)()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    status = (ctypes.c_int64 * 6)()

    def all_four(n, d, k):
        return [lib.gae_kmeans_workspace_bytes(n, d, k),
                lib.gae_kmeans_assign(p(X), d, n, d, p(X), k, p(out), None, p(X), 1 << 30, None),
                lib.gae_kmeans_step(p(X), d, n, d, p(X), k, p(out), p(status), 0.0, 0, p(X), 1 << 30, None),
                lib.gae_kmeans_init_pp(p(X), d, n, d, k, 0, p(X), p(out), p(X), 1 << 30, None)]
    assert all_four(100, 65, 3) == [GAE_E_RANGE] * 4 and b"d = 65" in lib.gae_last_error()
    assert all_four(100, 0, 3) == [GAE_E_RANGE] * 4
    assert all_four(1000, 16, 257) == [GAE_E_RANGE] * 4 and b"k = 257" in lib.gae_last_error()
    assert all_four(1000, 16, 0) == [GAE_E_RANGE] * 4
    assert all_four(-1, 16, 3) == [GAE_E_SIZE] * 4 and b"negative" in lib.gae_last_error()
    assert all_four(2, 16, 3) == [GAE_E_SIZE] * 4                      # k > n
    assert all_four(1 << 31, 16, 3) == [GAE_E_SIZE] * 4
    # a real shape: the remaining checks still come before any launch
    assert lib.gae_kmeans_assign(p(X), 15, 100, 16, p(X), 3, p(out), None, p(X), 1 << 30, None) == GAE_E_SIZE     # ldx < d
    assert lib.gae_kmeans_assign(None, 16, 100, 16, p(X), 3, p(out), None, p(X), 1 << 30, None) == -1
    assert lib.gae_kmeans_assign(p(X), 16, 100, 16, p(X), 3, p(out), None, p(X), 16, None) == -5           # short workspace
    assert lib.gae_kmeans_step(p(X), 16, 100, 16, p(X), 3, p(out), None, 0.0, 0, p(X), 1 << 30, None) == -1
    assert lib.gae_kmeans_step(p(X), 16, 100, 16, p(X), 3, p(out), p(status), 0.0, 4, p(X), 1 << 30, None) == GAE_E_RANGE
    assert lib.gae_kmeans_step(p(X), 16, 100, 16, p(X), 3, p(out), p(status), float("nan"), 0, p(X), 1 << 30,
                               None) == GAE_E_RANGE


def test_workspace_query_is_a_monotone_host_function(lib):
    last = 0
    for n in [256, 257, 1000, 4099, 32768, 32769, 40000, 131072, 131073, 200000, 249455, 10 ** 6, 10 ** 7, 2 ** 31 - 1]:
        b = lib.gae_kmeans_workspace_bytes(n, 48, 256)
        assert b >= last > -1 and b > 0, (n, b)
        last = b
    assert 0 < lib.gae_kmeans_workspace_bytes(1, 1, 1) <= lib.gae_kmeans_workspace_bytes(64, 1, 1) <= lib.gae_kmeans_workspace_bytes(65, 1, 1)
    assert lib.gae_kmeans_workspace_bytes(1, 1, 1) <= lib.gae_kmeans_workspace_bytes(33, 16, 3)
    assert lib.gae_kmeans_workspace_bytes(19717, 16, 3) < lib.gae_kmeans_workspace_bytes(19717, 64, 256)
    for bad in [(100, 65, 3), (100, 16, 257), (-5, 16, 3), (2, 16, 3), (100, 0, 3), (100, 16, 0)]:
        assert lib.gae_kmeans_workspace_bytes(*bad) < 0, bad
    # every n in a stretch around the point where the sums launch starts to grow its blocks' row ranges
    for lo in (32600, 130900):
        stretch = [lib.gae_kmeans_workspace_bytes(n, 16, 8) for n in range(lo, lo + 400)]
        assert all(a <= b for a, b in zip(stretch, stretch[1:]))


def test_kmeans_has_no_cpu_fallback(lib):
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    X = torch.randn(50, 8)
    with pytest.raises(GaeHipError):
        ops.kmeans(X, 3)
    with pytest.raises(GaeHipError):
        ops.kmeans_assign(X, X[:3])
    with pytest.raises(GaeHipError):
        ops.kmeans_init_pp(X, 3)
    with pytest.raises(ValueError):
        ops.kmeans(X, 3, max_iter=0)
    assert ops.KMeansResult._fields == ("labels", "centers", "counts", "inertia", "n_iter", "converged", "n_empty")
    import gae_dgl_amd as G
    from gae_dgl_amd.vgae import VGAE
    assert callable(G.GAE.cluster_nodes) and callable(VGAE.cluster_nodes)


# ------------------------------------------------------------------ clustering scores
def test_clustering_metrics_by_hand():
    from gae_dgl_amd.metrics import clustering_metrics
    true = np.array([0, 0, 0, 1, 1, 1, 2, 2, -1, -1])
    relabelled = np.array([7, 7, 7, 2, 2, 2, 5, 5, 0, 1])             # the ignored rows disagree on purpose
    assert clustering_metrics(relabelled, true) == {"nmi": 1.0, "ari": 1.0, "acc": 1.0, "n": 8}
    # the contingency table [[4, 0], [1, 5]]: rows = clusters, columns = classes, n = 10
    true = np.array([0] * 5 + [1] * 5)
    pred = np.array([0] * 4 + [1] * 6)
    m = clustering_metrics(pred, true)
    # ARI: sum_ij C(n_ij, 2) = 6 + 0 + 0 + 10 = 16; rows C(4,2) + C(6,2) = 21; columns 10 + 10 = 20; C(10,2) = 45;
    # expected 21 * 20 / 45 = 28/3; maximum (21 + 20) / 2 = 20.5
    assert m["ari"] == pytest.approx((16 - 28 / 3) / (20.5 - 28 / 3), abs=1e-12)
    # NMI: I = .4 ln(.4 / (.4 .5)) + .1 ln(.1 / (.6 .5)) + .5 ln(.5 / (.6 .5)); H(rows) = H(.4, .6); H(columns) = ln 2
    mi = 0.4 * np.log(2.0) + 0.1 * np.log(1 / 3) + 0.5 * np.log(5 / 3)
    h_rows = -(0.4 * np.log(0.4) + 0.6 * np.log(0.6))
    assert m["nmi"] == pytest.approx(mi / ((h_rows + np.log(2.0)) / 2), abs=1e-12)
    assert m["acc"] == pytest.approx(0.9) and m["n"] == 10
    # the matching is one to one: three clusters on two classes cannot all count
    m3 = clustering_metrics(np.array([0, 0, 1, 1, 2, 2]), np.array([0, 0, 0, 0, 1, 1]))
    assert m3["acc"] == pytest.approx(4 / 6)
    with_ignored = clustering_metrics(np.concatenate([pred, [1, 0, 1]]), np.concatenate([true, [-1, -1, -3]]))
    assert with_ignored == m
    assert np.isnan(clustering_metrics(np.array([1, 2]), np.array([-1, -1]))["nmi"])
    assert clustering_metrics(np.zeros(5, int), np.ones(5, int))["ari"] == 1.0      # one cluster, one class
    with pytest.raises(ValueError):
        clustering_metrics(np.zeros(3), np.zeros(4))


def test_clustering_metrics_against_sklearn_where_present():
    sm = pytest.importorskip("sklearn.metrics")
    from gae_dgl_amd.metrics import clustering_metrics
    rng = np.random.default_rng(1)
    for k_true, k_pred, n in ((3, 3, 200), (7, 5, 500), (2, 9, 64)):
        true, pred = rng.integers(0, k_true, n), rng.integers(0, k_pred, n)
        pred[: n // 2] = true[: n // 2] % k_pred
        m = clustering_metrics(pred, true)
        assert m["nmi"] == pytest.approx(sm.normalized_mutual_info_score(true, pred), abs=1e-10)
        assert m["ari"] == pytest.approx(sm.adjusted_rand_score(true, pred), abs=1e-10)


# ------------------------------------------------------------------ class labels of the citation data
def _planetoid_with_labels(tmp_path, with_labels):
    rng = np.random.default_rng(5)
    n_all, n, f, classes = 30, 41, 12, 4
    missing = {33}
    test_ids = np.asarray([i for i in range(n_all, n) if i not in missing])
    rng.shuffle(test_ids)                                              # a permuted test index
    feats = rng.integers(0, 3, (n, f)).astype(np.float32)
    adj = {u: [int(v) for v in rng.integers(0, n, 3) if int(v) not in missing] for u in range(n) if u not in missing}
    adj[33] = []
    y = rng.integers(0, classes, n)
    onehot = np.eye(classes, dtype=np.int32)[y]
    onehot[7] = 0                                                      # an unlabelled training node: all-zero row
    onehot[int(test_ids[2])] = 0                                       # ... and an unlabelled test node
    want = np.where(onehot.any(1), onehot.argmax(1), -1)
    want[33] = -1                                                      # no row in ty at all
    root = str(tmp_path / "citeseer")
    _write_planetoid(root, "citeseer", n_all, test_ids.tolist(), feats, adj)
    if with_labels:
        for ext, obj in (("ally", onehot[:n_all]), ("ty", onehot[test_ids])):
            with open(os.path.join(root, f"ind.citeseer.{ext}"), "wb") as fh:
                pickle.dump(obj, fh, protocol=2)
    return root, n, want


def test_labels_from_planetoid_files(tmp_path):
    from gae_dgl_amd import data as D
    root, n, want = _planetoid_with_labels(tmp_path, True)
    out = D.load_planetoid(root, "citeseer")
    assert len(out) == 4 and out[0] == n                               # the return shape existing callers unpack
    labels = D.load_planetoid_labels(root, "citeseer", n)
    assert labels.dtype == np.int64 and np.array_equal(labels, want)
    data = D.load_data(argparse.Namespace(dataset="citeseer", data_root=str(tmp_path)))
    assert np.array_equal(data.labels, want) and not data.synthetic
    os.remove(os.path.join(root, "ind.citeseer.ty"))                   # only one of the two files: no labels
    assert D.load_planetoid_labels(root, "citeseer", n) is None
    assert D.load_data(argparse.Namespace(dataset="citeseer", data_root=str(tmp_path))).labels is None


def test_labels_are_none_without_the_files(tmp_path):
    from gae_dgl_amd import data as D
    root, n, _ = _planetoid_with_labels(tmp_path, False)
    assert D.load_planetoid_labels(root, "citeseer", n) is None
    assert D.load_data(argparse.Namespace(dataset="citeseer", data_root=str(tmp_path))).labels is None
    assert D.CitationData("x", None, None, True).labels is None


def test_labels_from_an_npz(tmp_path):
    from gae_dgl_amd import data as D
    src, dst = np.array([0, 1, 2]), np.array([1, 2, 0])
    feats = np.eye(4, dtype=np.float32)
    np.savez(tmp_path / "cora.npz", src=src, dst=dst, features=feats, labels=np.array([2, 0, -1, 1], np.int32))
    data = D.load_data(argparse.Namespace(dataset="cora", data_root=str(tmp_path)))
    assert data.labels.dtype == np.int64 and data.labels.tolist() == [2, 0, -1, 1]
    np.savez(tmp_path / "pubmed.npz", src=src, dst=dst, features=feats)
    assert D.load_data(argparse.Namespace(dataset="pubmed", data_root=str(tmp_path))).labels is None


def test_script_flags_are_checked_before_any_device():
    from gae_dgl_amd import embed as E, train_transductive as TT
    args = TT.parse_args(["--cluster", "7", "--cluster_seed", "3", "--cluster_out", "c.npz"])
    assert (args.cluster, args.cluster_seed, args.cluster_out) == (7, 3, "c.npz")
    assert TT.parse_args([]).cluster is None
    for bad in (["--cluster", "0"], ["--cluster", "257"], ["--cluster_seed", "1"], ["--cluster_out", "x.npz"]):
        with pytest.raises(SystemExit):
            TT.parse_args(bad)
    base = ["--checkpoint", "c.pkl", "--hidden_dims", "32", "16", "--synthetic", "10", "--out", "f.npy"]
    assert E.parse_args(base + ["--clusters", "5"]).clusters == 5 and E.parse_args(base).clusters is None
    for bad in (base + ["--clusters", "300"], base + ["--clusters_out", "c.npz"],
                ["--checkpoint", "c.pkl", "--hidden_dims", "32", "--synthetic", "10", "--out", "f.npy", "--clusters", "2"]):
        with pytest.raises(SystemExit):
            E.parse_args(bad)


# ------------------------------------------------------------------ the reference against itself
def test_reference_philox_and_first_pick():
    ctr = np.array([0, 5, 2 ** 33 + 7])
    for draw, key in ((0, 1), (3, 0x1234567890ABCDEF), (2 ** 40, R.KEY_XOR)):
        words = R.philox_words(ctr, draw, key)
        assert [int(w) for w in words] == [philox4x32_10(int(c), draw, key)[0] for c in ctr]
    X = R.blobs(50, 4, 3)
    for seed in range(5):
        chosen, gaps = R.seed_pp(X, 3, seed)
        assert chosen[0] == philox4x32_10(0, 0, seed ^ R.KEY_XOR)[0] % 50 and len(gaps) == 2


def test_reference_seeding_is_d2_proportional():
    """the second centre over 4 000 seeds on an 8-point set: each point's frequency within 4 sigma of its D^2 share
    (averaged over the uniform first pick)"""
    rng = np.random.default_rng(11)
    X = rng.standard_normal((8, 2)).astype(np.float32) * np.array([3.0, 1.0], np.float32)
    D = R.dist2(X, X)
    expect = (D / D.sum(1, keepdims=True)).mean(0)                     # sum over the first pick of (1 / 8) D^2 share
    seeds = 4000
    hits, firsts = np.zeros(8), np.zeros(8)
    for seed in range(seeds):
        chosen, _ = R.seed_pp(X, 2, seed)
        firsts[chosen[0]] += 1
        hits[chosen[1]] += 1
    sigma = np.sqrt(expect * (1 - expect) / seeds)
    assert (np.abs(hits / seeds - expect) <= 4 * sigma).all(), (hits / seeds, expect)
    assert (np.abs(firsts / seeds - 1 / 8) <= 4 * np.sqrt(1 / 8 * 7 / 8 / seeds)).all()


def test_reference_gaps_of_the_gpu_cases():
    """the margins tests/test_gpu_kmeans.py relies on, computed in fp64: the seeding's best-to-second key gap over its
    four cases (smallest 1.5e-3) and the whole runs' best-to-second distance gap (smallest 5e-3)"""
    seed_gap = np.inf
    for n, d, k in ((33, 16, 3), (200, 16, 8), (257, 48, 5), (1000, 64, 33)):
        X = R.blobs(n, d, k, seed=1)
        for seed in range(20):
            chosen, gaps = R.seed_pp(X, k, seed)
            assert len(set(chosen.tolist())) == k
            seed_gap = min(seed_gap, float(gaps.min()))
    assert 1e-3 < seed_gap < 2e-3, seed_gap
    run_gap = np.inf
    for n, d, k in ((33, 16, 3), (200, 16, 8)):
        X = R.blobs(n, d, k, seed=1)
        tol_abs = 1e-4 * float(X.astype(np.float64).var(0).mean())
        for seed in range(20):
            run = R.lloyd(X, X[R.seed_pp(X, k, seed)[0]], tol_abs, 100)
            assert run["converged"] and run["n_iter"] <= 10
            run_gap = min(run_gap, run["gap"])
    assert 4e-3 < run_gap < 6e-3, run_gap


def test_reference_lloyd_rules():
    X = np.array([[0.0], [1.0], [10.0], [11.0], [5.5]], np.float32)
    # ties to the lower index; duplicate centres: the second never gets a row and keeps its value
    lab, d2, _ = R.assign(X, np.array([[0.0], [11.0], [0.0]]))
    assert lab.tolist() == [0, 0, 1, 1, 0] and d2.tolist() == [0.0, 1.0, 1.0, 0.0, 30.25]
    new, counts, n_empty, shift2 = R.update(X, lab, np.array([[0.0], [11.0], [0.0]]))
    assert counts.tolist() == [3, 2, 0] and n_empty == 1 and new[2, 0] == 0.0
    assert new[:, 0].tolist() == [6.5 / 3, 10.5, 0.0] and shift2 == pytest.approx((6.5 / 3) ** 2 + 0.25)
    run = R.lloyd(X, np.array([[0.0], [11.0]]), -1.0, 50)
    assert run["converged"] and run["changed"] == 0 and run["inertia"] == pytest.approx(sum((X[:, 0] - run["centers"][run["labels"], 0]) ** 2))
    assert not R.lloyd(X, np.array([[0.0], [1.0]]), -1.0, 1)["converged"]
    assert R.lloyd(X, np.array([[0.0], [1.0]]), 1e9, 50)["n_iter"] == 1          # shift2 <= tol_abs stops at once
