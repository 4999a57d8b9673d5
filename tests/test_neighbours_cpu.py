"""CPU-side checks of the neighbourhood baselines (K35 / K36): the numpy restatement against brute force on Python sets and
against a scipy.sparse int64 product, the closed forms on K_{7,5}, metrics.evaluate_scores, the new parser flags and the
argument errors of the C entry points (returned before anything is launched: no GPU needed)."""
import numpy as np
import pytest
import torch

import neighbour_ref as R


def _sets(n, src, dst):
    nb = [set() for _ in range(n)]
    for s, d in zip(src.tolist(), dst.tolist()):
        if s != d:
            nb[d].add(s)
    return nb


def test_reference_equals_brute_force_on_sets_and_a_sparse_product():
    import scipy.sparse as sp
    n = 60
    src, dst = R.random_graph(n, 110, 3)
    A = R.adjacency(n, src, dst)
    nb = _sets(n, src, dst)
    assert all(set(np.flatnonzero(A[i]).tolist()) == nb[i] for i in range(n))
    deg, W = R.weights(A)
    table = R.weight_table(int(deg.max()))
    assert table[0].tolist() == [0, 0] and table[1].tolist() == [0, 2 ** 32] and table[2, 1] == 2 ** 31
    assert table[2, 0] == int(np.rint(2.0 ** 32 / np.log(2.0)))
    # every pair, i == j included, against the sets
    pairs = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij")).reshape(2, -1)
    ps = R.pair_scores(A, pairs)
    for q in range(pairs.shape[1]):
        i, j = int(pairs[0, q]), int(pairs[1, q])
        both = nb[i] & nb[j]
        assert ps["common"][q] == len(both)
        assert ps["aa_sum"][q] == sum(int(table[len(nb[w]), 0]) for w in both)
        assert ps["ra_sum"][q] == sum(int(table[len(nb[w]), 1]) for w in both)
        union = len(nb[i] | nb[j])
        assert ps["union"][q] == union and ps["pa"][q] == len(nb[i]) * len(nb[j])
        assert ps["jaccard"][q] == (len(both) / union if union else 0.0)
    assert np.array_equal(ps["common"].reshape(n, n).diagonal(), deg)
    # the dense int64 route against scipy.sparse
    S = sp.csr_matrix(A.astype(np.int64))
    for kind, col in (("aa", 0), ("ra", 1)):
        common, wsum = R.two_hop(A, np.arange(n), kind)
        assert np.array_equal(common, (S @ S).toarray())
        assert np.array_equal(wsum, (S @ sp.diags(W[:, col]) @ S).toarray())
        assert np.array_equal(wsum.reshape(-1), ps[kind + "_sum"])
    # the candidate rule and the order against a sort of Python tuples
    for kind in R.KINDS:
        for exclude in (True, False):
            index, value, common, count = R.topk(A, 7, kind, exclude)
            key = {"cn": ps["cn"], "jaccard": ps["jaccard"], "aa": ps["aa_sum"], "ra": ps["ra_sum"]}[kind].reshape(n, n)
            for i in range(n):
                cand = [j for j in range(n) if j != i and nb[i] & nb[j] and not (exclude and j in nb[i])]
                best = sorted(cand, key=lambda j: (-key[i, j], j))[:7]
                assert count[i] == len(cand) and index[i, :len(best)].tolist() == best
                assert (index[i, len(best):] == -1).all() and np.isneginf(value[i, len(best):]).all()
                assert common[i, :len(best)].tolist() == [len(nb[i] & nb[j]) for j in best]


def test_closed_forms_on_a_complete_bipartite_graph():
    a, b = 7, 5
    left, right = np.arange(a), a + np.arange(b)
    s, d = np.repeat(left, b), np.tile(right, a)
    A = R.adjacency(a + b, np.concatenate([s, d]), np.concatenate([d, s]))
    pairs = np.stack(np.meshgrid(np.arange(a + b), np.arange(a + b), indexing="ij")).reshape(2, -1)
    ps = {k: v.reshape(a + b, a + b) for k, v in R.pair_scores(A, pairs).items()}
    assert (ps["common"][:a, :a] == b).all() and (ps["common"][a:, a:] == a).all()     # same side: the whole other side
    assert (ps["jaccard"][:a, :a] == 1.0).all() and (ps["jaccard"][a:, a:] == 1.0).all()
    assert (ps["common"][:a, a:] == 0).all() and (ps["common"][a:, :a] == 0).all()     # opposite sides share nobody
    # two nodes of the side of 7 share the 5 nodes of degree 7
    assert (ps["ra_sum"][:a, :a] == b * int(np.rint(2.0 ** 32 / 7))).all()
    assert (ps["aa_sum"][a:, a:] == a * int(np.rint(2.0 ** 32 / np.log(5.0)))).all()
    assert (ps["pa"][:a, a:] == a * b).all()
    index, value, common, count = R.topk(A, 10, "cn")
    assert (count[:a] == a - 1).all() and (count[a:] == b - 1).all()                     # the own side, minus the node
    assert index[0, :a - 1].tolist() == list(range(1, a)) and (index[0, a - 1:] == -1).all()


def test_evaluate_scores_equals_evaluate_on_sigmoid_scores():
    from gae_dgl_amd import metrics
    g = torch.Generator().manual_seed(0)
    Z = torch.randn(50, 8, generator=g)
    split = {"pos": torch.randint(0, 50, (2, 40), generator=g).numpy(), "neg": torch.randint(0, 50, (2, 60), generator=g).numpy()}
    want = metrics.evaluate(Z, split)
    got = metrics.evaluate_scores(metrics.edge_scores(Z, split["pos"]), metrics.edge_scores(Z, split["neg"]))
    assert got == want and 0.0 <= got["auc"] <= 1.0
    # integer scores with ties: the average-rank AUC
    got = metrics.evaluate_scores(torch.tensor([2, 1, 1]), torch.tensor([1, 0]))
    assert got["auc"] == (2 + 0.5 + 1 + 0.5 + 1) / 6


def test_parser_takes_the_heuristics_flags_and_refuses_bad_combinations(capsys):
    from gae_dgl_amd import train_transductive as TT
    args = TT.parse_args(["--eval", "--heuristics"])
    assert args.heuristics == [] and args.heuristics_out is None
    args = TT.parse_args(["--eval", "--heuristics", "aa", "pa", "--topk", "10", "--heuristics_out", "h.npz"])
    assert args.heuristics == ["aa", "pa"] and args.topk == 10 and args.heuristics_out == "h.npz"
    assert TT.parse_args([]).heuristics is None
    assert TT.HEURISTIC_KINDS == ("cn", "jaccard", "aa", "ra", "pa")
    for argv, text in ((["--heuristics"], "--heuristics needs --eval"),
                       (["--eval", "--heuristics_out", "h.npz"], "--heuristics_out needs --heuristics"),
                       (["--eval", "--heuristics", "katz"], "invalid choice")):
        with pytest.raises(SystemExit) as e:
            TT.parse_args(argv)
        assert e.value.code == 2 and text in capsys.readouterr().err


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    import ctypes
    from gae_dgl_amd import _lib, ops
    lib = _lib.load()
    NULL, SIZE, WORKSPACE, RANGE = -1, -2, -5, -6
    buf = ctypes.create_string_buffer(4096)                 # host memory: every call below returns before a launch
    p = ctypes.addressof(buf)
    err = lambda: lib.gae_last_error().decode()

    assert lib.gae_neighbour_degrees(None, p, 4, 8, p, p, None) == NULL and "indptr" in err()
    assert lib.gae_neighbour_degrees(p, None, 4, 8, p, p, None) == NULL and "indices" in err()
    assert lib.gae_neighbour_degrees(p, p, 4, 8, None, p, None) == NULL and "deg" in err()
    assert lib.gae_neighbour_degrees(p, p, 4, 8, p, None, None) == NULL and "status" in err()
    assert lib.gae_neighbour_degrees(p, p, -1, 8, p, p, None) == SIZE and "negative" in err()
    assert lib.gae_neighbour_degrees(p, p, 4, -8, p, p, None) == SIZE
    assert lib.gae_neighbour_degrees(p, p, 1 << 30, 8, p, p, None) == SIZE and "2^30" in err()
    assert lib.gae_neighbour_degrees(p, p, 4, 1 << 31, p, p, None) == SIZE
    assert lib.gae_neighbour_degrees(p, None, 0, 0, None, p, None) == 0      # an empty graph: nothing to launch

    pairs = lambda **kw: lib.gae_neighbour_pairs(*[kw.get(k, v) for k, v in (
        ("indptr", p), ("indices", p), ("n", 4), ("nnz", 8), ("pi", p), ("pj", p), ("m", 3), ("W", p), ("nw", 2), ("common", p),
        ("wsum", p), ("status", p), ("stream", None))])
    for name in ("indptr", "indices", "pi", "pj", "W", "common", "wsum", "status"):
        assert pairs(**{name: None}) == NULL, name
    assert pairs(m=-1) == SIZE and pairs(n=-4) == SIZE and pairs(n=1 << 30) == SIZE and pairs(m=1 << 31) == SIZE
    assert pairs(nw=3) == RANGE and pairs(nw=-1) == RANGE
    assert pairs(m=0) == 0 and pairs(nw=0, W=None, wsum=None, m=0) == 0

    assert lib.gae_neighbour_topk_workspace_bytes(300, 300) > 0
    assert lib.gae_neighbour_topk_workspace_bytes(300, 300) <= lib.gae_neighbour_topk_workspace_bytes(300, 3000)
    assert lib.gae_neighbour_topk_workspace_bytes(-1, 3) == SIZE and lib.gae_neighbour_topk_workspace_bytes(3, -1) == SIZE
    assert lib.gae_neighbour_topk_workspace_bytes(1 << 30, 3) == SIZE
    need = lib.gae_neighbour_topk_workspace_bytes(4, 4)
    assert need <= 4096
    topk = lambda **kw: lib.gae_neighbour_topk(*[kw.get(k, v) for k, v in (
        ("indptr", p), ("indices", p), ("n", 4), ("nnz", 8), ("rows", None), ("m", 4), ("k", 10), ("kind", _lib.NEIGHBOUR_AA),
        ("w", p), ("ldw", 2), ("deg", p), ("flags", 1), ("table_slots", 0), ("index", p), ("common", p), ("wsum", p),
        ("status", p), ("ws", p), ("ws_bytes", need), ("stream", None))])
    for name in ("indptr", "indices", "w", "deg", "index", "common", "wsum", "status", "ws"):
        assert topk(**{name: None}) == NULL, name
    assert topk(k=0) == RANGE and topk(k=65) == RANGE and "1..64" in err()
    assert topk(kind=4) == RANGE and "pa" in err() and topk(kind=-1) == RANGE
    for slots in (48, 100, 32, 4096, -64):
        assert topk(table_slots=slots) == RANGE and "power of two" in err(), slots
    assert topk(flags=2) == RANGE
    assert topk(n=-1) == SIZE and topk(m=-1) == SIZE and topk(n=1 << 30) == SIZE and topk(ldw=0) == SIZE
    assert topk(ws_bytes=need - 1) == WORKSPACE
    assert topk(m=0) == 0 and topk(m=0, kind=_lib.NEIGHBOUR_CN, w=None) == 0

    # the mirror of the constants, and the wrappers' own refusals
    assert (_lib.NEIGHBOUR_SCALE_BITS, _lib.NEIGHBOUR_TABLE_SLOTS) == (32, 1024) == (ops.NEIGHBOUR_SCALE_BITS, ops.NEIGHBOUR_TABLE_SLOTS)
    header = open(_lib.HERE + "/../include/gae_hip_experimental.h").read()
    for name in ("SCALE_BITS", "TABLE_SLOTS", "MAX_K", "CN", "JACCARD", "AA", "RA", "EXCLUDE_EDGES", "ERR_COLUMN", "ERR_ORDER",
                 "ERR_QUERY", "ERR_TABLE", "ERR_INDPTR", "STATUS_WORDS"):
        assert f"GAE_NEIGHBOUR_{name} = {getattr(_lib, 'NEIGHBOUR_' + name)}" in header, name
    assert np.array_equal(ops.neighbour_weight_table(40), R.weight_table(40))
    import gae_dgl_amd as G
    g = G.DGLGraph(([0, 1], [1, 0]), num_nodes=3)
    with pytest.raises(_lib.GaeHipError):
        ops.neighbour_weights(g)
    with pytest.raises(_lib.GaeHipError):
        ops.neighbour_scores(g, torch.zeros(2, 1, dtype=torch.int64))
    with pytest.raises(_lib.GaeHipError):
        ops.neighbour_topk(g, 3, "pa")
    with pytest.raises(_lib.GaeHipError):
        ops.neighbour_topk(g, 3, "aa")
