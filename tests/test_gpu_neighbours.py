"""K35 / K36 on the device (ops.neighbour_scores, ops.neighbour_topk) against the numpy restatement of the header comment
(tests/neighbour_ref.py), bit for bit: every pair of a random graph with duplicate edges and self-loops, the closed forms,
every kind x k x exclude_edges of the top-k on two graphs, both routes, the cross-invariant between the two entry points,
determinism, the refusals and one train_transductive --heuristics run."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import neighbour_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GRAPHS = {"sparse": (300, 450, 2), "dense": (300, 900, 1)}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    return got.shape == want.shape and np.array_equal(_bits(got), _bits(want.astype(got.dtype)))


def _graph(n, src, dst):
    import gae_dgl_amd as G
    return G.DGLGraph((np.asarray(src, np.int64), np.asarray(dst, np.int64)), num_nodes=n).to(DEV)


@functools.lru_cache(maxsize=None)
def _random(name):
    n, u, seed = GRAPHS[name]
    src, dst = R.random_graph(n, u, seed)
    return n, src, dst, R.adjacency(n, src, dst), _graph(n, src, dst)


@functools.lru_cache(maxsize=None)
def _ref_topk(name, kind, exclude):
    """the 64 best of every row, computed once: the k best are its first k columns"""
    return R.topk(_random(name)[3], 64, kind, exclude)


def _check_scores(got, want):
    for field in got._fields:
        assert _same(getattr(got, field), want[field]), field
    assert got.common.dtype == torch.int32 and got.pa.dtype == torch.int64 and got.jaccard.dtype == torch.float64
    assert got.aa_sum.dtype == torch.int64 and got.aa.dtype == torch.float64


def _all_pairs(n):
    return np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij")).reshape(2, -1)


# ------------------------------------------------------------------------------------------------------------ pairs
def test_every_pair_of_a_random_graph_with_duplicates_and_self_loops():
    from gae_dgl_amd import ops
    n, src, dst, A, g = _random("sparse")
    assert len(src) > len(np.unique(src * n + dst)) and (src == dst).any()          # duplicates and self-loops are in it
    pairs = _all_pairs(n)                                                          # i == j included
    want = R.pair_scores(A, pairs)
    deg, W = ops.neighbour_weights(g)
    assert _same(deg, A.sum(1)) and _same(W, R.weights(A)[1])
    _check_scores(ops.neighbour_scores(g, torch.from_numpy(pairs).to(DEV)), want)
    _check_scores(ops.neighbour_scores(g, torch.from_numpy(pairs.astype(np.int32)).to(DEV), weights=(deg, W)), want)
    assert (want["common"] > 1).any() and (want["union"] == 0).any()


def test_pairs_on_a_complete_bipartite_graph_a_path_and_an_edgeless_graph():
    from gae_dgl_amd import ops
    a, b = 7, 5
    s, d = np.repeat(np.arange(a), b), np.tile(a + np.arange(b), a)
    cases = [(a + b, np.concatenate([s, d]), np.concatenate([d, s])),
             (9, np.concatenate([np.arange(8), np.arange(1, 9)]), np.concatenate([np.arange(1, 9), np.arange(8)])),
             (6, np.zeros(0, np.int64), np.zeros(0, np.int64))]
    for n, src, dst in cases:
        A = R.adjacency(n, src, dst)
        pairs = _all_pairs(n)
        got = ops.neighbour_scores(_graph(n, src, dst), torch.from_numpy(pairs).to(DEV))
        _check_scores(got, R.pair_scores(A, pairs))
        if n == a + b:
            common = got.common.cpu().numpy().reshape(n, n)
            assert (common[:a, :a] == b).all() and (common[a:, a:] == a).all() and (common[:a, a:] == 0).all()
            assert (got.jaccard.cpu().numpy().reshape(n, n)[:a, :a] == 1.0).all()
            assert (got.ra_sum.cpu().numpy().reshape(n, n)[:a, :a] == b * int(np.rint(2.0 ** 32 / 7))).all()
        if len(src) == 0:
            assert not got.common.any() and not got.jaccard.any() and not got.pa.any()
            top = ops.neighbour_topk(_graph(n, src, dst), 3, "cn")
            assert (top.index == -1).all() and torch.isneginf(top.value).all()


def test_pairs_on_a_star_search_the_long_row_for_the_short_one():
    from gae_dgl_amd import ops
    leaves = 5000
    hub = 0
    src = np.concatenate([np.zeros(leaves, np.int64), 1 + np.arange(leaves)])
    dst = src[::-1].copy()
    n = leaves + 1
    g = _graph(n, src, dst)
    rng = np.random.default_rng(0)
    pi = np.concatenate([np.full(200, hub), 1 + rng.integers(0, leaves, 200), 1 + rng.integers(0, leaves, 300), [hub]])
    pj = np.concatenate([1 + rng.integers(0, leaves, 200), np.full(200, hub), 1 + rng.integers(0, leaves, 300), [hub]])
    pairs = np.stack([pi, pj])
    got = ops.neighbour_scores(g, torch.from_numpy(pairs).to(DEV))
    _check_scores(got, R.pair_scores(R.adjacency(n, src, dst), pairs))
    common = got.common.cpu().numpy()
    assert (common[:400] == 0).all()                                   # hub - leaf: the hub is no neighbour of itself
    leaf_leaf = common[400:700]
    assert ((leaf_leaf == 1) | (pi[400:700] == pj[400:700])).all() and common[700] == leaves


def test_a_pair_outside_the_graph_gives_minus_one_and_raises_through_the_status():
    from gae_dgl_amd import _lib, ops
    from gae_dgl_amd.ops import _ptr, _stream
    n, src, dst, A, g = _random("sparse")
    for bad in (n, -1):
        with pytest.raises(_lib.GaeHipError, match="query index"):
            ops.neighbour_scores(g, torch.tensor([[0, 3], [5, bad]], device=DEV))
    with pytest.raises(_lib.GaeHipError, match="query index"):
        ops.neighbour_topk(g, 3, "cn", rows=torch.tensor([1, n], device=DEV))
    indptr, indices = g.csr()
    deg, W = ops.neighbour_weights(g)
    pi = torch.tensor([0, 3, 7], dtype=torch.int32, device=DEV)
    pj = torch.tensor([5, n, 9], dtype=torch.int32, device=DEV)
    common = torch.zeros(3, dtype=torch.int32, device=DEV)
    wsum = torch.zeros(3, 2, dtype=torch.int64, device=DEV)
    status = torch.zeros(_lib.NEIGHBOUR_STATUS_WORDS, dtype=torch.int64, device=DEV)
    _lib.call("gae_neighbour_pairs", _ptr(indptr), _ptr(indices), n, indices.numel(), _ptr(pi), _ptr(pj), 3, _ptr(W), 2,
              _ptr(common), _ptr(wsum), _ptr(status), _stream())
    want = R.pair_scores(A, np.array([[0, 7], [5, 9]]))["common"]
    assert common.tolist() == [want[0], -1, want[1]] and int(status[0]) == _lib.NEIGHBOUR_ERR_QUERY


# ------------------------------------------------------------------------------------------------------------ top-k
def test_the_random_graphs_have_the_rows_the_topk_tests_need():
    """preconditions, on the reference: isolated rows, rows with fewer than 10 candidates, rows with more, and rows whose
    10th place is tied -- so that padding, the cut and the order by j are all exercised"""
    A = _random("sparse")[3]
    for kind in ("cn", "aa"):
        count = _ref_topk("sparse", kind, True)[3]
        assert (count == 0).sum() > 0 and ((count > 0) & (count < 10)).sum() > 0 and (count > 10).sum() > 0
        assert len(R.tied_rows(A, 10, kind)) > 0
    assert (_ref_topk("dense", "cn", True)[3] > 64).sum() > 0 or (_ref_topk("dense", "cn", False)[3] > 64).sum() > 0


@pytest.mark.parametrize("exclude", [True, False])
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_topk_equals_the_reference(name, kind, k, exclude):
    from gae_dgl_amd import ops
    g = _random(name)[4]
    index, value, common, _ = _ref_topk(name, kind, exclude)
    got = ops.neighbour_topk(g, k, kind, exclude_edges=exclude)
    assert got.index.dtype == torch.int32 and got.value.dtype == torch.float64 and got.common.dtype == torch.int32
    assert _same(got.index, index[:, :k]) and _same(got.value, value[:, :k]) and _same(got.common, common[:, :k])


# ------------------------------------------------------------------------------------------------------------ routes
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_small_tables_force_the_long_route_and_keep_every_bit(name, kind):
    from gae_dgl_amd import ops
    n, _, _, _, g = _random(name)
    index, value, common, count = _ref_topk(name, kind, True)
    base = ops.neighbour_topk(g, 64, kind)
    short, long_ = ops.neighbour_last_routes()
    assert short > 0 and short + long_ == int((_random(name)[3].sum(1) > 0).sum())  # every row that has a neighbour
    small = ops.neighbour_topk(g, 64, kind, table_slots=64)
    assert ops.neighbour_last_routes()[1] > long_                                  # rows moved to the long route
    for a, b, want in zip(base, small, (index, value, common)):
        assert _same(a, want) and _same(b, want)
    mid = ops.neighbour_topk(g, 10, kind, table_slots=256)
    assert _same(mid.index, index[:, :10]) and _same(mid.value, value[:, :10])


def test_two_hubs_that_share_a_table_of_leaves_take_the_long_route_by_default():
    from gae_dgl_amd import ops
    L = ops.NEIGHBOUR_TABLE_SLOTS
    leaves = 2 + np.arange(L)
    src = np.concatenate([np.zeros(L, np.int64), np.ones(L, np.int64), leaves, leaves, [5, 9]])
    dst = np.concatenate([leaves, leaves, np.zeros(L, np.int64), np.ones(L, np.int64), [9, 5]])
    n = L + 2
    A = R.adjacency(n, src, dst)
    g = _graph(n, src, dst)
    rows = np.array([0, 1, 2, 5, 9, L + 1, 700])
    for kind in R.KINDS:
        for exclude in (True, False):
            index, value, common, count = R.topk(A, 64, kind, exclude, rows=rows)
            got = ops.neighbour_topk(g, 64, kind, rows=torch.from_numpy(rows).to(DEV), exclude_edges=exclude)
            assert ops.neighbour_last_routes() == (0, len(rows))                   # B = 2 L + ... > L / 2 for every row
            assert _same(got.index, index) and _same(got.value, value) and _same(got.common, common)
    count = R.topk(A, 1, "cn", True, rows=rows)[3]
    assert count[0] == 1 and count[2] == L - 1                                     # the other hub; every other leaf


# ------------------------------------------------------------------------------------------------- cross-invariant
@pytest.mark.parametrize("kind", R.KINDS)
def test_topk_values_are_the_pair_scores_of_their_pairs(kind):
    from gae_dgl_amd import ops
    n, _, _, _, g = _random("dense")
    top = ops.neighbour_topk(g, 10, kind, exclude_edges=False)
    valid = top.index >= 0
    i = torch.arange(n, device=DEV).unsqueeze(1).expand_as(top.index)[valid]
    ps = ops.neighbour_scores(g, torch.stack([i, top.index[valid].long()]))
    assert valid.any() and torch.equal(top.common[valid], ps.common)
    assert torch.equal(top.value[valid].view(torch.int64), getattr(ps, kind).double().view(torch.int64))


# ------------------------------------------------------------------------------------------------------ determinism
def test_runs_streams_row_subsets_and_permutations_give_the_same_rows():
    from gae_dgl_amd import ops
    n, _, _, _, g = _random("dense")
    for kind, slots in (("aa", 0), ("jaccard", 64)):
        first = ops.neighbour_topk(g, 10, kind, table_slots=slots)
        again = ops.neighbour_topk(g, 10, kind, table_slots=slots)
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            other = ops.neighbour_topk(g, 10, kind, table_slots=slots)
        stream.synchronize()
        perm = torch.from_numpy(np.random.default_rng(1).permutation(n)).to(DEV)
        shuffled = ops.neighbour_topk(g, 10, kind, rows=perm, table_slots=slots)
        subset = perm[:37].to(torch.int32)
        part = ops.neighbour_topk(g, 10, kind, rows=subset, table_slots=slots)
        for f in range(3):
            assert torch.equal(first[f], again[f]) and torch.equal(first[f], other[f]) and torch.equal(first[f][perm], shuffled[f])
            assert torch.equal(first[f][subset.long()], part[f])


# ----------------------------------------------------------------------------------------------------------- errors
def test_refusals_and_the_flags_of_a_broken_graph():
    from gae_dgl_amd import _lib, ops
    from gae_dgl_amd.ops import _ptr, _stream
    g = _graph(4, [0, 1, 2], [1, 0, 3])                                            # 2 -> 3 has no mirror
    for call in (lambda: ops.neighbour_weights(g), lambda: ops.neighbour_topk(g, 2, "cn"),
                 lambda: ops.neighbour_scores(g, torch.zeros(2, 1, dtype=torch.int64, device=DEV))):
        with pytest.raises(_lib.GaeHipError, match="not symmetric"):
            call()
    good = _random("sparse")[4]
    with pytest.raises(_lib.GaeHipError, match="pa"):
        ops.neighbour_topk(good, 5, "pa")
    for k in (0, 65):
        with pytest.raises(_lib.GaeHipError):
            ops.neighbour_topk(good, k, "cn")
    with pytest.raises(_lib.GaeHipError, match="power of two"):
        ops.neighbour_topk(good, 5, "cn", table_slots=100)
    with pytest.raises(_lib.GaeHipError):
        ops.neighbour_scores(good, torch.zeros(2, 1, dtype=torch.int64))             # a CPU tensor

    def flags(indptr, indices):
        indptr = torch.tensor(indptr, dtype=torch.int32, device=DEV)
        indices = torch.tensor(indices, dtype=torch.int32, device=DEV)
        n = indptr.numel() - 1
        deg = torch.zeros(n, dtype=torch.int32, device=DEV)
        status = torch.zeros(_lib.NEIGHBOUR_STATUS_WORDS, dtype=torch.int64, device=DEV)
        _lib.call("gae_neighbour_degrees", _ptr(indptr), _ptr(indices), n, indices.numel(), _ptr(deg), _ptr(status), _stream())
        return int(status[0]), deg.tolist()
    assert flags([0, 2, 4, 6], [1, 2, 0, 2, 0, 1]) == (0, [2, 2, 2])
    assert flags([0, 3, 5, 7], [1, 1, 2, 0, 1, 0, 2]) == (0, [2, 1, 1])              # a duplicate, two self-loops
    assert flags([0, 2, 4, 6], [2, 1, 0, 2, 0, 1]) == (_lib.NEIGHBOUR_ERR_ORDER, [2, 2, 2])
    assert flags([0, 2, 4, 6], [1, 3, 0, 2, 0, 1])[0] == _lib.NEIGHBOUR_ERR_COLUMN
    assert flags([0, 2, 4, 6], [-1, 2, 0, 2, 0, 1])[0] == _lib.NEIGHBOUR_ERR_COLUMN
    assert flags([0, 2, 9, 6], [1, 2, 0, 2, 0, 1])[0] & _lib.NEIGHBOUR_ERR_INDPTR


# -------------------------------------------------------------------------------------------------------------- CLI
def test_train_transductive_prints_the_heuristic_lines(tmp_path):
    from gae_dgl_amd import metrics, ops
    rng = np.random.default_rng(0)
    n, c = 300, 5
    comm = rng.integers(0, c, n)
    a, b = rng.integers(0, n, 6000), rng.integers(0, n, 6000)
    keep = ((comm[a] == comm[b]) | (rng.random(a.size) < 0.03)) & (a != b)
    a, b = a[keep], b[keep]
    feats = np.eye(c, dtype=np.float32)[comm] + 0.1 * rng.standard_normal((n, c)).astype(np.float32)
    os.makedirs(tmp_path / "data")
    src, dst = np.concatenate([a, b]), np.concatenate([b, a])
    np.savez(tmp_path / "data" / "cora.npz", src=src, dst=dst, features=feats, n=n)
    out = tmp_path / "pairs.npz"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "gae_dgl_amd.train_transductive", "--dataset", "cora", "--data_root",
                        str(tmp_path / "data"), "-e", "3", "-s", str(tmp_path), "--seed", "0", "--log_every", "100", "--no_hipgraph",
                        "--eval", "--heuristics", "--topk", "10", "--heuristics_out", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert any(re.fullmatch(r"test ROC-AUC: [\d.]+ \| AP: [\d.]+", l) for l in lines)       # the model's own line is still there
    kept, val, test = metrics.split_edges(src, dst, n, seed=0)
    g = _graph(n, kept[0], kept[1])
    tables = np.load(out)
    for name, split in (("val", val), ("test", test)):
        ns = {part: ops.neighbour_scores(g, torch.from_numpy(split[part]).to(DEV)) for part in ("pos", "neg")}
        for kind in ("cn", "jaccard", "aa", "ra", "pa"):
            want = metrics.evaluate_scores(getattr(ns["pos"], kind), getattr(ns["neg"], kind))
            assert f"{kind} {name} ROC-AUC: {want['auc']:.4f} | AP: {want['ap']:.4f}" in lines, (kind, name)
            for part in ("pos", "neg"):
                assert _same(getattr(ns[part], kind), tables[f"{name}_{part}_{kind}"])
        assert np.array_equal(tables[f"{name}_pos_pairs"], split["pos"])
    # held-out edges lie mostly inside a community, random non-edges mostly across two: the baseline must beat chance
    assert metrics.evaluate_scores(ns["pos"].aa, ns["neg"].aa)["auc"] > 0.5
    for kind in ("cn", "jaccard", "aa", "ra"):
        recall = metrics.recall_at_k(ops.neighbour_topk(g, 10, kind).index, test["pos"])
        assert f"{kind} test recall@10: {recall:.4f}" in lines
    assert not any(l.startswith("pa test recall") for l in lines)
