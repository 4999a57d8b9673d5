"""K37 / K38 without a GPU: the numpy restatement (tests/deepwalk_ref.py) against the properties the contract states -- walks
step along stored entries, a sink ends a walk, a walk depends on its id and its start only, the noise table -- the host
side of ops.deepwalk (weights, argument errors of the library and of the wrappers, the parser) and the learning condition
of the synchronous Adagrad schedule on the two-block graph."""
import functools

import numpy as np
import pytest

import deepwalk_ref as R


@functools.lru_cache(maxsize=None)
def _walks():
    n, src, dst = R.walk_graph()
    indptr, indices = R.csr(n, src, dst)
    return n, indptr, indices, R.random_walks(indptr, indices, None, 3, 9, seed=5)


def test_every_step_is_a_stored_entry_of_the_row_before_it():
    n, indptr, indices, walks = _walks()
    assert walks.shape == (3 * n, 9) and walks.dtype == np.int32
    assert np.array_equal(walks[:, 0], np.tile(np.arange(n), 3))
    assert indptr[70] - indptr[69] == 300
    stepped = 0
    for w in walks:
        for t in range(1, 9):
            if w[t - 1] < 0:
                assert w[t] == -1
            elif indptr[w[t - 1] + 1] == indptr[w[t - 1]]:
                assert w[t] == -1
            else:
                assert w[t] in indices[indptr[w[t - 1]]:indptr[w[t - 1] + 1]]
                stepped += 1
    assert stepped > 1000
    assert len({tuple(w) for w in walks[[5, 75, 145]]}) > 1                       # the repeats of a start differ


def test_a_sink_ends_the_walk_with_minus_ones():
    n, indptr, indices, walks = _walks()
    for node in (67, 68):
        assert indptr[node + 1] == indptr[node]
        for rep in range(3):
            assert walks[rep * n + node].tolist() == [node] + [-1] * 8
    reached = [w for w in walks if 68 in w[1:]]                                    # 68 is a source of rows 1, 2, 5
    assert reached
    for w in reached:
        at = list(w).index(68)
        assert (w[at + 1:] == -1).all()


def test_a_walk_depends_on_its_id_and_its_start_only():
    n, indptr, indices, _ = _walks()
    one = R.random_walks(indptr, indices, [10, 20, 30], 2, 12, seed=3)
    two = R.random_walks(indptr, indices, [40, 20, 50], 2, 12, seed=3)
    assert np.array_equal(one[[1, 4]], two[[1, 4]])                                # same id, same start
    assert not np.array_equal(one[0], two[0])
    swapped = R.random_walks(indptr, indices, [20, 10, 30], 2, 12, seed=3)
    assert not np.array_equal(one[1], swapped[0])                                  # same start, another id: another stream
    assert not np.array_equal(one, R.random_walks(indptr, indices, [10, 20, 30], 2, 12, seed=4))
    short = R.random_walks(indptr, indices, [10, 20, 30], 2, 5, seed=3)
    assert np.array_equal(short, one[:, :5])                                       # a longer walk continues a shorter one


def test_the_noise_table_never_draws_an_unvisited_node():
    walks = np.asarray([[0, 3, 3, 7, -1], [7, 7, 9, -1, -1]], np.int32)
    cum = R.noise_table(walks, 12, 0.75)
    counts = R.counts_of(walks, 12)
    assert counts.tolist() == [1, 0, 0, 2, 0, 0, 0, 3, 0, 1, 0, 0]
    assert cum[0] == 0 and (np.diff(cum) > 0).tolist() == (counts > 0).tolist()
    drawn = R.negatives(cum, 11, 2, np.arange(200), 64)
    assert drawn.shape == (200, 64) and set(np.unique(drawn)) == {0, 3, 7, 9}
    freq = np.bincount(drawn.reshape(-1), minlength=12) / drawn.size
    want = np.diff(cum) / cum[-1]
    assert np.abs(freq - want).max() < 0.02                                        # 12800 draws: sd below 0.005
    assert not np.array_equal(drawn, R.negatives(cum, 11, 3, np.arange(200), 64))   # the epoch is in the key
    assert np.array_equal(drawn[:, :16], R.negatives(cum, 11, 2, np.arange(200), 16))


def test_power_zero_and_power_one_give_the_stated_tables():
    from gae_dgl_amd import ops
    walks = np.asarray([[0, 3, 3, 7, -1], [7, 7, 9, -1, -1]], np.int32)
    counts = R.counts_of(walks, 10)
    assert np.diff(R.noise_table(walks, 10, 0.0)).tolist() == [2 ** 20 if c else 0 for c in counts]
    assert np.diff(R.noise_table(walks, 10, 1.0)).tolist() == [2 ** 20 * c for c in counts]
    for power in (0.0, 0.5, 0.75, 1.0):
        assert np.array_equal(ops.sgns_noise_weights(counts, power), np.diff(R.noise_table(walks, 10, power)))
    assert np.diff(R.noise_table(walks, 10, 0.75))[7] == int(np.rint(2.0 ** 20 * 3.0 ** 0.75))


def test_argument_errors_of_the_library_do_not_need_a_gpu():
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    lib = _lib.load()
    E_NULL, E_SIZE, E_RANGE = -1, -2, -6
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def accumulate(L=20, d=16, window=5, K=5, M=16, n_walks=4, first=0, count=4, epoch=0, n=3, ptr=p):
        return lib.gae_sgns_accumulate(ptr, n_walks, L, ptr, first, count, ptr, n, d, window, K, M, 0, epoch, ptr, ptr, ptr, ptr,
                                       ptr, None)
    assert accumulate(d=129) == E_RANGE and b"d = 129" in lib.gae_last_error()
    assert accumulate(d=0) == E_RANGE
    assert accumulate(L=65, window=5) == E_RANGE and b"length = 65" in lib.gae_last_error()
    assert accumulate(L=1, window=1) == E_RANGE
    assert accumulate(M=20) == E_RANGE and b"shared_negatives = 20" in lib.gae_last_error()
    assert accumulate(L=20, window=20) == E_RANGE and b"window = 20" in lib.gae_last_error()
    assert accumulate(window=0) == E_RANGE
    assert accumulate(K=-1) == E_RANGE and accumulate(K=1025) == E_RANGE
    assert accumulate(epoch=-1) == E_RANGE
    assert accumulate(first=2, count=3) == E_SIZE and accumulate(n=0) == E_SIZE and accumulate(n_walks=0) == E_SIZE
    assert accumulate(ptr=None) == E_NULL
    assert accumulate(count=0) == 0                                                 # an empty batch launches nothing

    f = ctypes.c_float
    assert lib.gae_sgns_update(p, p, p, p, p, p, 3, 129, f(0.05), f(1e-8), p, None) == E_RANGE
    assert lib.gae_sgns_update(p, p, p, p, p, p, 3, 16, f(0.0), f(1e-8), p, None) == E_RANGE
    assert lib.gae_sgns_update(p, p, p, p, p, p, 3, 16, f(0.05), f(float("nan")), p, None) == E_RANGE
    assert lib.gae_sgns_update(p, None, p, p, p, p, 3, 16, f(0.05), f(1e-8), p, None) == E_NULL
    assert lib.gae_sgns_init(None, 3, 16, 0, f(0.1), None) == E_NULL and lib.gae_sgns_init(p, 3, 200, 0, f(0.1), None) == E_RANGE
    assert lib.gae_sgns_walk_order(-1, 0, 0, p, None) == E_SIZE and lib.gae_sgns_walk_order(5, 0, -1, p, None) == E_RANGE
    assert lib.gae_sgns_walk_order(5, 0, 0, None, None) == E_NULL

    def walks(n=3, nnz=4, starts=None, m=3, r=2, L=5, ptr=p, out=p):
        return lib.gae_random_walks(ptr, ptr, n, nnz, starts, m, r, L, 0, out, ptr, None)
    assert walks(L=0) == E_RANGE and walks(L=65537) == E_RANGE and b"length = 65537" in lib.gae_last_error()
    assert walks(r=0) == E_RANGE
    assert walks(n=-1) == E_SIZE and walks(m=4) == E_SIZE and walks(m=2 ** 20, r=2 ** 12, starts=p) == E_SIZE
    assert walks(ptr=None) == E_NULL and walks(out=None) == E_NULL
    assert walks(m=0) == 0


def test_argument_errors_of_the_wrappers():
    import torch
    import gae_dgl_amd as G
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    g = G.DGLGraph()
    g.add_nodes(3)
    g.add_edges([0, 1], [1, 2])
    with pytest.raises(GaeHipError):
        ops.random_walks(g)                                                         # a CPU graph: no fallback
    with pytest.raises(GaeHipError):
        ops.deepwalk(g, 8)
    for bad in (dict(walk_length=0), dict(walk_length=2 ** 16 + 1), dict(walks_per_node=0), dict(seed=-1), dict(walk_length=2.5)):
        with pytest.raises(GaeHipError):
            ops.random_walks(g, **bad)
    for dim in (0, 129, True, 2.0):
        with pytest.raises(GaeHipError):
            ops.deepwalk(g, dim)
    with pytest.raises(GaeHipError):
        ops.sgns_noise_table(torch.zeros(2, 3, dtype=torch.int32), 4)               # a CPU tensor
    with pytest.raises(GaeHipError):
        ops.sgns_init(4, 8, device="cpu")
    t = torch.zeros(4, 8)
    with pytest.raises(GaeHipError):
        ops.sgns_train(torch.zeros(2, 3, dtype=torch.int32), torch.zeros(5, dtype=torch.int64), t, t, t, t)
    assert ops.DeepWalkResult._fields == ("embedding", "context", "walks", "counts", "n_batches", "info")


def test_parser_errors():
    from gae_dgl_amd.train_transductive import parse_args
    ok = parse_args(["--eval", "--deepwalk", "16", "--deepwalk_walks", "4", "--deepwalk_length", "12", "--deepwalk_window", "3",
                     "--deepwalk_epochs", "2", "--deepwalk_seed", "9", "--deepwalk_out", "dw.npz"])
    assert (ok.deepwalk, ok.deepwalk_walks, ok.deepwalk_length, ok.deepwalk_window, ok.deepwalk_epochs, ok.deepwalk_seed,
            ok.deepwalk_out) == (16, 4, 12, 3, 2, 9, "dw.npz")
    assert parse_args(["--eval"]).deepwalk is None
    for argv in (["--deepwalk", "16"],                                             # needs --eval
                 ["--eval", "--deepwalk", "0"], ["--eval", "--deepwalk", "129"],
                 ["--eval", "--deepwalk_walks", "4"], ["--eval", "--deepwalk_length", "12"], ["--eval", "--deepwalk_window", "3"],
                 ["--eval", "--deepwalk_epochs", "2"], ["--eval", "--deepwalk_seed", "1"], ["--eval", "--deepwalk_out", "x.npz"],
                 ["--eval", "--deepwalk", "16", "--deepwalk_walks", "0"],
                 ["--eval", "--deepwalk", "16", "--deepwalk_length", "1"], ["--eval", "--deepwalk", "16", "--deepwalk_length", "65"],
                 ["--eval", "--deepwalk", "16", "--deepwalk_window", "0"],
                 ["--eval", "--deepwalk", "16", "--deepwalk_length", "5", "--deepwalk_window", "5"],
                 ["--eval", "--deepwalk", "16", "--deepwalk_epochs", "0"], ["--eval", "--deepwalk", "16", "--deepwalk_seed", "-1"]):
        with pytest.raises(SystemExit):
            parse_args(argv)


def test_the_trainer_masks_invalid_positions_and_own_negatives():
    """one walk with a -1 tail: its invalid positions get no gradient, a negative equal to the row's own node has coefficient
    +0, and K = 0 leaves the negatives' rows untouched"""
    rng = np.random.default_rng(1)
    n, d = 6, 4
    W = (rng.random((n, d)).astype(np.float32) - 0.5)
    C = (rng.random((n, d)).astype(np.float32) - 0.5)
    ids = np.asarray([[2, 4, 2, -1, -1]], np.int64)
    neg = np.asarray([[2, 5, 1, 0] * 4], np.int64)
    dW, dC, valid = R.batch_grads(ids, neg, W, C, 2, 3)
    assert valid.tolist() == [[True, True, True, False, False]]
    assert not dW[0, 3:].any() and not dC[0, 3:5].any()
    assert dW[0, :3].any() and dC[0, 5:].any()
    dW0, dC0, _ = R.batch_grads(ids, neg, W, C, 2, 0)
    assert not dC0[0, 5:].any() and dW0[0, :3].any()
    only_own = np.full((1, 16), 4, np.int64)                                       # every negative is node 4 = position 1
    _, dC1, _ = R.batch_grads(ids, only_own, W, C, 2, 3)
    Gn_row1_free = R.batch_grads(np.asarray([[4, 4, 4, -1, -1]], np.int64), only_own, W, C, 2, 3)[1]
    assert dC1[0, 5:].any() and not Gn_row1_free[0, 5:].any()


def test_the_learning_condition_on_the_two_block_graph():
    """2 x 32 nodes, p_in 0.3, p_out 0.02 (numpy seed 0); d = 16, r = 10, L = 20, window 5, K = 5, M = 16, 3 epochs of batches
    of 64 walks at lr 0.05: the same-block ROC-AUC of the cosine similarity over all node pairs must reach 0.9.
    The restatement gives 0.9810 (the float64 prototype of the schedule gave 0.99 - 1.00 with other random streams)."""
    n, src, dst, block = R.two_blocks(0)
    indptr, indices = R.csr(n, src, dst)
    st, walks, cum = R.deepwalk(indptr, indices, 16, walks_per_node=10, walk_length=20, window=5, negatives_per_pair=5,
                                shared_negatives=16, epochs=3, batch_walks=64, lr=0.05, seed=0)
    assert walks.shape == (640, 20) and st.n_batches == 30 and st.flags == 0
    assert not st.AW.any() and not st.AC.any()
    value = R.same_block_auc(st.W, block)
    print(f"same-block ROC-AUC {value:.4f}")
    assert value >= 0.9
