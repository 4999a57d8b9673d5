"""K37 / K38 on the device (ops.random_walks, ops.sgns_train, ops.deepwalk) against the numpy restatement of the header
comment (tests/deepwalk_ref.py), bit for bit: the walks on a graph with an isolated node, a sink row and a hub row, the
start table and the walk order, the four tables after two epochs on every tile shape, -1 tails, short last batches, a star
whose centre takes every atomic, K = 0, a second run and a non-default stream, the refusals and one train_transductive
--deepwalk run."""
import functools
import os

import numpy as np
import pytest
import torch

import deepwalk_ref as R
import mlp_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_RANGE = -6


def _same(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    if got.shape != want.shape:
        return False
    if got.dtype == np.float32:
        return np.array_equal(got.view(np.int32), want.astype(np.float32).view(np.int32))
    return np.array_equal(got, want.astype(got.dtype))


def _graph(n, src, dst):
    import gae_dgl_amd as G
    return G.DGLGraph((np.asarray(src, np.int64), np.asarray(dst, np.int64)), num_nodes=n).to(DEV)


@functools.lru_cache(maxsize=None)
def _walk_graph():
    n, src, dst = R.walk_graph()
    indptr, indices = R.csr(n, src, dst)
    return n, indptr, indices, _graph(n, src, dst)


@functools.lru_cache(maxsize=None)
def _star():
    leaves = 30
    a, b = np.zeros(leaves, np.int64), 1 + np.arange(leaves)
    src, dst = np.concatenate([a, b]), np.concatenate([b, a])
    indptr, indices = R.csr(leaves + 1, src, dst)
    return leaves + 1, indptr, indices, _graph(leaves + 1, src, dst)


# ------------------------------------------------------------------------------------------------------------ walks
def test_the_device_csr_is_the_restatements():
    n, indptr, indices, g = _walk_graph()
    d_indptr, d_indices = g.csr()
    assert _same(d_indptr, indptr) and _same(d_indices, indices)
    assert indptr[68] == indptr[67] and indptr[69] == indptr[68] and indptr[70] - indptr[69] == 300


@pytest.mark.parametrize("L", [2, 5, 9, 64])
def test_walks_match_the_restatement(L):
    from gae_dgl_amd import ops
    n, indptr, indices, g = _walk_graph()
    want = R.random_walks(indptr, indices, None, 3, L, seed=5)
    got = ops.random_walks(g, walks_per_node=3, walk_length=L, seed=5)
    assert got.dtype == torch.int32 and _same(got, want)
    assert (want[:, -1] == -1).any() and (want[:, -1] >= 0).any()
    assert _same(ops.random_walks(g, walks_per_node=3, walk_length=L, seed=5), want)          # the same bits again
    assert not _same(ops.random_walks(g, walks_per_node=3, walk_length=L, seed=6), want)


def test_walks_from_a_start_subset():
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    n, indptr, indices, g = _walk_graph()
    starts = [69, 3, 67, 3, 68, 40, 12]
    want = R.random_walks(indptr, indices, starts, 3, 9, seed=2)
    for dtype in (torch.int64, torch.int32):
        assert _same(ops.random_walks(g, walks_per_node=3, walk_length=9, starts=torch.tensor(starts, dtype=dtype, device=DEV),
                                      seed=2), want)
    assert not np.array_equal(want[1], want[3])                                    # the same start under two ids
    with pytest.raises(GaeHipError, match="a start outside"):
        ops.random_walks(g, walk_length=4, starts=torch.tensor([1, 70], device=DEV))
    with pytest.raises(GaeHipError):
        ops.random_walks(g, walk_length=4, starts=torch.tensor([1, 2]))             # a CPU tensor


def test_the_start_table_and_the_walk_order_match_the_restatement():
    from gae_dgl_amd import _lib, ops
    from gae_dgl_amd.ops import _ptr, _stream
    for n, dim, seed in ((70, 16, 0), (33, 5, 9)):
        assert _same(ops.sgns_init(n, dim, seed=seed, device=DEV), R.init_table(n, dim, seed))
    for n_walks, seed, epoch in ((1, 0, 0), (140, 3, 0), (140, 3, 1), (1000, 2 ** 40 + 7, 5)):
        order = torch.empty(n_walks, dtype=torch.int32, device=DEV)
        _lib.call("gae_sgns_walk_order", n_walks, seed, epoch, _ptr(order), _stream())
        assert _same(order, mlp_ref.perm(n_walks, seed, epoch))


def test_the_noise_table_matches_the_restatement():
    from gae_dgl_amd import ops
    n, indptr, indices, g = _walk_graph()
    walks = R.random_walks(indptr, indices, None, 2, 9, seed=1)
    for power in (0.0, 0.75, 1.0):
        got = ops.sgns_noise_table(torch.from_numpy(walks).to(DEV), n, power)
        assert got.dtype == torch.int64 and _same(got, R.noise_table(walks, n, power))


# ------------------------------------------------------------------------------------------------------------ trainer
def _device_train(walks, cum, W, C, HW, HC, *, window, K, M, epochs, batch, lr, eps, seed):
    """the wrapper's loop with the accumulators in view: (W, C, HW, HC, AW, AC, status word 0)"""
    from gae_dgl_amd import _lib
    from gae_dgl_amd.ops import _ptr, _stream
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(DEV)
    walks_d, cum_d = t(walks, torch.int32), t(cum, torch.int64)
    W, C, HW, HC = (t(a, torch.float32) for a in (W, C, HW, HC))
    n, d = W.shape
    n_walks, L = walks.shape
    AW, AC = (torch.zeros(n, d, dtype=torch.int64, device=DEV) for _ in range(2))
    order = torch.empty(n_walks, dtype=torch.int32, device=DEV)
    status = torch.zeros(_lib.DEEPWALK_STATUS_WORDS, dtype=torch.int64, device=DEV)
    for epoch in range(epochs):
        _lib.call("gae_sgns_walk_order", n_walks, seed, epoch, _ptr(order), _stream())
        for first in range(0, n_walks, batch):
            _lib.call("gae_sgns_accumulate", _ptr(walks_d), n_walks, L, _ptr(order), first, min(batch, n_walks - first),
                      _ptr(cum_d), n, d, window, K, M, seed, epoch, _ptr(W), _ptr(C), _ptr(AW), _ptr(AC), _ptr(status), _stream())
            _lib.call("gae_sgns_update", _ptr(W), _ptr(C), _ptr(HW), _ptr(HC), _ptr(AW), _ptr(AC), n, d,
                      float(np.float32(lr)), float(np.float32(eps)), _ptr(status), _stream())
    return W, C, HW, HC, AW, AC, int(status.cpu()[0])


def _start_state(n, d, seed):
    """a start with every table in play: W from the library's draw, C a second draw, positive Adagrad sums"""
    W = R.init_table(n, d, seed)
    C = R.init_table(n, d, seed + 1)
    HW = np.abs(R.init_table(n, d, seed + 2))
    HC = np.zeros((n, d), np.float32)
    return W, C, HW, HC


# (L, d, M, window), walks per start, starts (None: every node), batch: the batch never divides the walk count
SHAPES = {"5-4-16-1": ((5, 4, 16, 1), 2, None, 37), "20-16-16-5": ((20, 16, 16, 5), 2, None, 37),
          "17-20-32-16": ((17, 20, 32, 16), 1, None, 16), "64-128-64-10": ((64, 128, 64, 10), 1, [0, 5, 67, 9, 68, 69, 30], 3)}


@functools.lru_cache(maxsize=None)
def _case(name, K=5, seed=0):
    (L, d, M, window), r, starts, batch = SHAPES[name]
    n, indptr, indices, _ = _walk_graph()
    walks = R.random_walks(indptr, indices, starts, r, L, seed=11)
    assert (walks[:, 1:] == -1).any() and walks.shape[0] % batch != 0               # -1 tails, a short last batch
    cum = R.noise_table(walks, n, 0.75)
    start = _start_state(n, d, seed)
    kw = dict(window=window, shared_negatives=M, epochs=2, lr=0.05, eps=1e-8, seed=seed)
    want = R.train(walks, cum, *start, negatives_per_pair=K, batch_walks=batch, **kw)
    assert want.flags == 0
    return walks, cum, start, dict(window=window, K=K, M=M, epochs=2, batch=batch, lr=0.05, eps=1e-8, seed=seed), want


def _check_state(got, want):
    for name, g, w in zip(("W", "C", "HW", "HC"), got[:4], (want.W, want.C, want.HW, want.HC)):
        assert _same(g, w), name
    assert not bool(got[4].any()) and not bool(got[5].any())                        # the accumulators are zero again
    assert got[6] == 0


@pytest.mark.parametrize("name", list(SHAPES))
def test_two_epochs_match_the_restatement(name):
    walks, cum, start, kw, want = _case(name)
    got = _device_train(walks, cum, *start, **kw)
    _check_state(got, want)
    assert not _same(got[0], start[0]) and not _same(got[1], start[1])
    untouched = R.counts_of(walks, start[0].shape[0]) == 0                           # rows no walk visits keep their values
    assert untouched.any() == (SHAPES[name][2] is not None)
    for g, before in zip(got[:4], start):
        assert _same(g[torch.from_numpy(untouched).to(DEV)], before[untouched])


def test_a_second_run_and_a_side_stream_give_the_same_bits():
    walks, cum, start, kw, want = _case("20-16-16-5")
    _check_state(_device_train(walks, cum, *start, **kw), want)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = _device_train(walks, cum, *start, **kw)
    side.synchronize()
    _check_state(got, want)


def test_no_negatives_per_pair_and_another_seed():
    walks, cum, start, kw, want = _case("20-16-16-5", K=0, seed=3)
    got = _device_train(walks, cum, *start, **kw)
    _check_state(got, want)
    assert not _same(got[0], _case("20-16-16-5")[4].W)


def test_a_star_whose_centre_is_in_every_walk():
    """every walk alternates centre and leaf: one row of W and of C takes an atomic from every walk of the batch"""
    n, indptr, indices, _ = _star()
    walks = R.random_walks(indptr, indices, None, 4, 8, seed=1)
    assert (walks == 0).any(axis=1).all()
    cum = R.noise_table(walks, n, 0.75)
    start = _start_state(n, 16, 5)
    want = R.train(walks, cum, *start, window=3, negatives_per_pair=5, shared_negatives=16, epochs=2, batch_walks=walks.shape[0],
                   lr=0.05, eps=1e-8, seed=5)
    got = _device_train(walks, cum, *start, window=3, K=5, M=16, epochs=2, batch=walks.shape[0], lr=0.05, eps=1e-8, seed=5)
    _check_state(got, want)


def test_the_wrappers_match_the_restatement():
    """ops.sgns_train in place on the caller's tables, and ops.deepwalk from the graph to the embedding"""
    from gae_dgl_amd import ops
    walks, cum, start, kw, want = _case("20-16-16-5")
    W, C, HW, HC = (torch.from_numpy(a.copy()).to(DEV) for a in start)
    nb = ops.sgns_train(torch.from_numpy(walks).to(DEV), torch.from_numpy(cum).to(DEV), W, C, HW, HC, window=kw["window"],
                        negatives=kw["K"], shared_negatives=kw["M"], epochs=2, batch_walks=kw["batch"], lr=0.05, eps=1e-8, seed=0)
    assert nb == want.n_batches
    for name, g, w in zip(("W", "C", "HW", "HC"), (W, C, HW, HC), (want.W, want.C, want.HW, want.HC)):
        assert _same(g, w), name

    n, indptr, indices, g = _walk_graph()
    args = dict(walks_per_node=2, walk_length=12, window=4, shared_negatives=32, epochs=2, batch_walks=50, lr=0.05, seed=4)
    st, ref_walks, ref_cum = R.deepwalk(indptr, indices, 8, negatives_per_pair=3, **args)
    res = ops.deepwalk(g, 8, negatives=3, **args)
    assert _same(res.walks, ref_walks) and _same(res.counts, R.counts_of(ref_walks, n)) and res.n_batches == st.n_batches
    assert _same(res.embedding, st.W) and _same(res.context, st.C)
    assert _same(res.info["hw"], st.HW) and _same(res.info["hc"], st.HC)
    assert res.info["n_walks"] == 2 * n and res.info["visited"] == int((R.counts_of(ref_walks, n) > 0).sum())
    given = ops.deepwalk(g, 8, negatives=3, walks=res.walks, **args)                # a given walk table
    assert _same(given.embedding, st.W)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    from gae_dgl_amd import _lib, ops
    from gae_dgl_amd._lib import GaeHipError
    from gae_dgl_amd.ops import _ptr
    lib = _lib.load()
    n = 12
    buf = torch.zeros(4096, dtype=torch.int64, device=DEV)
    p = _ptr(buf)

    def accumulate(L=20, d=16, window=5, M=16):
        return lib.gae_sgns_accumulate(p, 4, L, p, 0, 4, p, n, d, window, 5, M, 0, 0, p, p, p, p, p, None)
    assert accumulate(d=129) == E_RANGE and b"d = 129 outside 1..128" in lib.gae_last_error()
    assert accumulate(L=65) == E_RANGE and b"length = 65 outside 2..64" in lib.gae_last_error()
    assert accumulate(M=20) == E_RANGE and b"shared_negatives = 20 is not 16, 32, 48 or 64" in lib.gae_last_error()
    assert accumulate(L=20, window=20) == E_RANGE and b"window = 20 outside 1..length - 1" in lib.gae_last_error()

    walks = torch.tensor([[0, 1, 2, 3, -1], [4, 5, 4, 5, 4]], dtype=torch.int32, device=DEV)
    cum = ops.sgns_noise_table(walks, n)
    tables = lambda d=8: [ops.sgns_init(n, d, device=DEV)] + [torch.zeros(n, d, device=DEV) for _ in range(3)]
    for bad in (dict(shared_negatives=20), dict(window=5), dict(window=0), dict(negatives=-1)):
        with pytest.raises(GaeHipError):
            ops.sgns_train(walks, cum, *tables(), **bad)
    with pytest.raises(GaeHipError):
        ops.sgns_train(torch.zeros(2, 65, dtype=torch.int32, device=DEV), cum, *tables())
    with pytest.raises(GaeHipError):
        ops.sgns_train(walks, cum, *[torch.zeros(n, 129, device=DEV) for _ in range(4)])
    for which in range(2):                                                        # a table holding an inf
        t = tables()
        t[which][4, 3] = float("inf")
        with pytest.raises(GaeHipError, match="non-finite"):
            ops.sgns_train(walks, cum, *t)
    with pytest.raises(GaeHipError, match="walk-table entry"):
        ops.sgns_train(torch.tensor([[0, 12, 1]], dtype=torch.int32, device=DEV), cum, *tables(), window=2)
    with pytest.raises(GaeHipError):
        ops.sgns_train(walks, torch.zeros(n + 1, dtype=torch.int64, device=DEV), *tables())   # an empty noise table
    with pytest.raises(GaeHipError):
        ops.sgns_train(walks.cpu(), cum, *tables())
    huge = tables()
    huge[0].fill_(3.0e5)                                                           # finite tables, a gradient beyond 2^20
    huge[1].fill_(-3.0e5)
    with pytest.raises(GaeHipError, match="2\\^20"):
        ops.sgns_train(walks, cum, *huge, window=4, epochs=1)


# ------------------------------------------------------------------------------------------------------------ the script
def test_train_transductive_prints_the_baseline(tmp_path, capsys):
    import gae_dgl_amd as G
    from gae_dgl_amd import metrics, ops
    from gae_dgl_amd import train_transductive as TT
    n, src, dst, block = R.two_blocks(1, size=40, p_in=0.3, p_out=0.02)
    feats = np.random.default_rng(3).standard_normal((n, 12)).astype(np.float32)
    os.makedirs(tmp_path / "data", exist_ok=True)
    np.savez(tmp_path / "data" / "cora.npz", src=src, dst=dst, features=feats, n=n, labels=block)
    TT.main(["--dataset", "cora", "--data_root", str(tmp_path / "data"), "-e", "3", "-s", str(tmp_path), "--seed", "0",
             "--log_every", "100", "--eval", "--deepwalk", "16", "--deepwalk_walks", "4", "--deepwalk_length", "12",
             "--deepwalk_window", "3", "--deepwalk_epochs", "2", "--deepwalk_seed", "7", "--deepwalk_out", str(tmp_path / "dw.npz")])
    out = capsys.readouterr().out
    assert "deepwalk (16) val ROC-AUC: " in out and "deepwalk (16) test ROC-AUC: " in out
    for line in out.splitlines():                                                  # the model's own lines are printed as before
        assert line.startswith("deepwalk") or "deepwalk" not in line
    assert "\ntest ROC-AUC: " in out and "\nval ROC-AUC: " in out
    last = TT.main.last_deepwalk
    saved = np.load(tmp_path / "dw.npz")
    assert saved["embedding"].shape == (n, 16) and _same(last["result"].embedding, saved["embedding"])

    kept, val, test = metrics.split_edges(src.tolist(), dst.tolist(), n, seed=0)
    g = G.DGLGraph(kept, num_nodes=n).to(DEV)
    again = ops.deepwalk(g, 16, walks_per_node=4, walk_length=12, window=3, epochs=2, seed=7)
    assert _same(again.embedding, saved["embedding"])
    for name, pairs in (("val", val), ("test", test)):
        scores = metrics.evaluate(again.embedding, pairs)
        assert scores["auc"] == last[name]["auc"] and scores["ap"] == last[name]["ap"]
        assert f"deepwalk (16) {name} ROC-AUC: {scores['auc']:.4f} | AP: {scores['ap']:.4f}" in out
