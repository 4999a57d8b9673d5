"""K27 on the device (gae_mlp_fit, gae_mlp_predict, ops.mlp, GAE.mlp_graphs, the embed script) against the numpy
restatement tests/mlp_ref.py: weights, moments, loss curves and held-out errors bit for bit.

Shapes are the smallest that reach each path: one row tile and two (a panel is 32 rows), one panel and several, widths
that are no multiple of the 16-wide tile, column tiles on one wave and on two (more than 64 units), one hidden layer and
two, a short last batch, a batch larger than the list.

The forward and backward maps run on quarter-grid data: every product and every partial sum is exact in fp32 (the test
asserts the bound), so the expected values do not depend on the order of any sum and a transposed or mis-rowed tile
cannot hide behind rounding."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mlp_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
HEADER = 16
CANARY = 12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    from gae_dgl_amd import _lib
    assert _lib.MLP_STATE_HEADER == HEADER
    return torch.device("cuda:0")


def as_np(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def state_floats(d, hidden, t):
    from gae_dgl_amd import _lib
    h2 = hidden[1] if len(hidden) > 1 else 0
    return int(_lib.load().gae_mlp_workspace_bytes(d, hidden[0], h2, t, 1)) // 4


def unpack(block, d, hidden, t):
    """(W, b, mW, mb, vW, vb, step, b1p, b2p, info, epochs_done) of one state block (fp32 numpy [S])"""
    shapes = R.layer_shapes(d, hidden, t)
    P = sum(o * i + o for o, i in shapes)
    sets = []
    for k in range(3):
        o0, Ws, bs = HEADER + k * P, [], []
        for out, inn in shapes:
            Ws.append(block[o0:o0 + out * inn].reshape(out, inn).copy()); o0 += out * inn
            bs.append(block[o0:o0 + out].copy()); o0 += out
        sets += [Ws, bs]
    head = block[:HEADER].copy()
    return (*sets, int(head.view(np.int64)[0]), float(head.view(np.float64)[1]), float(head.view(np.float64)[2]),
            int(head.view(np.int32)[6]), int(head.view(np.int32)[7]))


def pack(W, b, d, hidden, t, epochs_done=0):
    """a state block with these weights, zero moments, step 0"""
    block = np.zeros(state_floats(d, hidden, t), np.float32)
    o = HEADER
    for w, v in zip(W, b):
        block[o:o + w.size] = w.reshape(-1); o += w.size
        block[o:o + v.size] = v; o += v.size
    block[:HEADER].view(np.float64)[1:3] = 1.0
    block[:HEADER].view(np.int32)[7] = epochs_done
    return block


def guarded(arr, dev, pad=0, fill=NAN):
    """(view, whole): `arr` on the device as a [n, w] view into rows `pad` wider that hold `fill`, or as it is"""
    t = torch.from_numpy(np.ascontiguousarray(arr))
    if not pad:
        return t.to(dev), None
    whole = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype)
    whole[:, :t.shape[1]] = t
    whole = whole.to(dev)
    return whole[:, :t.shape[1]], whole


def with_canary(shape, dtype, dev):
    """(view, whole): an output of `shape` with 64 canary elements behind it"""
    n = int(np.prod(shape))
    whole = torch.full((n + 64,), CANARY, dtype=dtype, device=dev)
    return whole[:n].reshape(shape), whole


def intact(whole, n):
    return bool((whole[n:] == CANARY).all())


def run_fit(dev, X, Y, hidden, lists, train, evals, lrs, alphas, seeds, *, shift=None, scale=None, epochs=3, batch_size=8,
            solver=0, momentum=0.0, shuffle=True, cuts=None, padx=0, pady=0, state=None, first_epoch=0):
    """gae_mlp_fit on numpy inputs; `lists`: row-id arrays; `cuts`: epochs per launch (None: one launch); `state`: start
    from these blocks at `first_epoch`.  Returns (blocks fp32 [M, S], loss_curve, eval_sse, info, status) as numpy, with
    the canaries behind every output and the workspace checked."""
    from gae_dgl_amd import _lib
    from gae_dgl_amd.ops import _ptr, _stream
    X = np.asarray(X, np.float32)
    Y = np.asarray(Y, np.float32).reshape(len(X), -1)
    n, d = X.shape
    t = Y.shape[1]
    M = len(train)
    S = state_floats(d, hidden, t)
    Xd, _ = guarded(X, dev, padx)
    Yd, _ = guarded(Y, dev, pady)
    rows = torch.tensor(np.concatenate([np.asarray(l, np.int32) for l in lists]), dtype=torch.int32, device=dev)
    ptr = torch.tensor(np.concatenate([[0], np.cumsum([len(l) for l in lists])]), dtype=torch.int32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    tr, ev = torch.tensor(train, **i32), torch.tensor(evals, **i32)
    lr = torch.tensor(lrs, dtype=torch.float32, device=dev)
    al = torch.tensor(alphas, dtype=torch.float32, device=dev)
    sd = torch.tensor(seeds, dtype=torch.int64, device=dev)
    sh = None if shift is None else torch.tensor(shift, dtype=torch.float32, device=dev)
    sc = None if scale is None else torch.tensor(scale, dtype=torch.float32, device=dev)
    total = first_epoch + epochs
    loss, loss_w = with_canary((M, total), torch.float64, dev)
    sse, sse_w = with_canary((M, t), torch.float64, dev)
    info, info_w = with_canary((M,), torch.int32, dev)
    ws, ws_w = with_canary((M, S), torch.float32, dev)
    if state is not None:
        ws.copy_(torch.from_numpy(np.asarray(state, np.float32)).to(dev))
    status = torch.zeros(4, dtype=torch.int64, device=dev)
    h2 = hidden[1] if len(hidden) > 1 else 0
    step = cuts or epochs
    for e0 in range(first_epoch, total, step):
        e1 = min(total, e0 + step)
        flags = (_lib.MLP_SHUFFLE if shuffle else 0) | (_lib.MLP_FINAL if e1 == total else 0)
        _lib.call("gae_mlp_fit", _ptr(Xd), Xd.stride(0) if n > 1 else d + padx, _ptr(Yd), Yd.stride(0) if n > 1 else t + pady, n,
                  d, hidden[0], h2, t, _ptr(sh), _ptr(sc), _ptr(rows), rows.numel(), _ptr(ptr), len(lists), _ptr(tr), _ptr(ev),
                  _ptr(lr), _ptr(al), _ptr(sd), M, batch_size, 0.9, 0.999, 1e-8, solver, momentum, flags, e0, e1, total,
                  _ptr(loss), _ptr(sse), _ptr(info), _ptr(status), _ptr(ws), M * S * 4, _stream())
    torch.cuda.synchronize()
    assert intact(loss_w, M * total) and intact(sse_w, M * t) and intact(info_w, M) and intact(ws_w, M * S)
    return as_np(ws), as_np(loss)[:, first_epoch:], as_np(sse), as_np(info), as_np(status)


def check_model(block, loss, sse, info, ref, d, hidden, t):
    W, b, mW, mb, vW, vb, step, b1p, b2p, inf, done = unpack(block, d, hidden, t)
    assert inf == ref.info == info and step == ref.step
    assert b1p == ref.b1p and b2p == ref.b2p
    for l in range(len(W)):
        for name, got, want in (("W", W, ref.W), ("b", b, ref.b), ("mW", mW, ref.mW), ("mb", mb, ref.mb), ("vW", vW, ref.vW),
                                ("vb", vb, ref.vb)):
            assert same_bits(got[l], want[l]), (name, l, np.abs(got[l] - want[l]).max())
    assert same_bits(loss, ref.loss_curve), (loss, ref.loss_curve)
    assert same_bits(sse, ref.eval_sse), (sse, ref.eval_sse)


# ------------------------------------------------------------------ 1. the forward and backward maps on grid data
def grid_net(rng, d, hidden, t):
    """quarter-grid weights whose size shrinks layer by layer (|w| <= 1, 1/2, 1/4), asymmetric by construction"""
    W, b = [], []
    for l, (out, inn) in enumerate(R.layer_shapes(d, hidden, t)):
        top = 4 >> l
        W.append((rng.integers(-top, top + 1, (out, inn)) / 4).astype(np.float32))
        b.append((rng.integers(-top, top + 1, out) / 4).astype(np.float32))
    return W, b


def exact_forward(W, b, X):
    """fp64 activations, with the assertion that every partial sum of every chain is exact in fp32"""
    a, acts, unit = X.astype(np.float64), [], 4.0
    for l in range(len(W)):
        acts.append(a)
        unit *= 4.0
        worst = (np.abs(a) @ np.abs(W[l].astype(np.float64)).T + np.abs(b[l])).max()
        assert worst * unit < 2 ** 24, (l, worst * unit)
        a = a @ W[l].astype(np.float64).T + b[l]
        if l < len(W) - 1:
            a = np.maximum(a, 0.0)
    return acts, a


LADDER = [  # n, d, hidden, t: every n, d, h and t of the ladder at least once
    (1, 1, (1,), 1), (63, 4, (16,), 3), (64, 5, (17,), 8), (65, 48, (100,), 1), (200, 128, (128,), 8), (65, 5, (64, 64), 3),
    (63, 48, (17, 33), 1), (200, 4, (128,), 1), (64, 48, (16,), 8),
]


@pytest.mark.parametrize("n,d,hidden,t", LADDER)
def test_forward_map_is_exact_on_grid_data(n, d, hidden, t, dev):
    from gae_dgl_amd import _lib
    from gae_dgl_amd.ops import _ptr, _stream
    rng = np.random.default_rng(n * 1000 + d)
    X = (rng.integers(-4, 5, (n, d)) / 4).astype(np.float32)
    nets = [grid_net(rng, d, hidden, t) for _ in range(2)]
    blocks = np.stack([pack(W, b, d, hidden, t) for W, b in nets])
    Xd, whole = guarded(X, dev, 3)
    out, out_w = with_canary((2, n, t), torch.float32, dev)
    st = torch.from_numpy(blocks).to(dev)
    _lib.call("gae_mlp_predict", _ptr(Xd), Xd.stride(0) if n > 1 else d + 3, n, d, hidden[0], hidden[1] if len(hidden) > 1 else 0,
              t, None, None, _ptr(st), 2, _ptr(out), None, _stream())
    torch.cuda.synchronize()
    assert intact(out_w, 2 * n * t)
    for k, (W, b) in enumerate(nets):
        _, want = exact_forward(W, b, X)
        assert np.array_equal(as_np(out[k]).astype(np.float64), want), k
        assert same_bits(as_np(out[k]), R.predict_rows(W, b, X))


@pytest.mark.parametrize("n,d,hidden,t", LADDER)
def test_backward_map_is_exact_on_grid_data(n, d, hidden, t, dev):
    """one SGD step without momentum or penalty from a state block written by hand, lr = 2^-6, one batch of all n rows,
    no shuffle: w' = w - lr (dW / n) shows every element of every gradient; dW itself is exact on the grid"""
    rng = np.random.default_rng(n * 1000 + d + 1)
    X = (rng.integers(-4, 5, (n, d)) / 4).astype(np.float32)
    Y = (rng.integers(-8, 9, (n, t)) / 4).astype(np.float32)
    W, b = grid_net(rng, d, hidden, t)
    acts, out = exact_forward(W, b, X)
    lr = 2.0 ** -6
    ref = R.fit(X, Y, hidden, np.arange(n), lr=lr, alpha=0.0, epochs=1, batch_size=256, solver=R.SGD, shuffle=False,
                init=(W, b), first_epoch=1)
    blocks, loss, sse, info, status = run_fit(dev, X, Y, hidden, [np.arange(n)], [0], [-1], [lr], [0.0], [0], epochs=1,
                                              batch_size=256, solver=1, shuffle=False, padx=1, pady=2,
                                              state=pack(W, b, d, hidden, t, 1)[None], first_epoch=1)
    assert status.tolist() == [0, 0, 0, 0] and info.tolist() == [0]
    gW, gb = unpack(blocks[0], d, hidden, t)[:2]
    for l in range(len(W)):
        assert same_bits(gW[l], ref.W[l]), (l, np.abs(gW[l] - ref.W[l]).max())
        assert same_bits(gb[l], ref.b[l]), l
    # the output layer's gradient against plain fp64 numpy: its sums are exact in fp32 (units: 4^-(L + 1) for the
    # error, 4^-L for the activation): one division, one product, one subtraction follow
    d_out = out - Y
    exact = (np.abs(d_out).T @ np.abs(acts[-1])).max() * 4.0 ** (2 * len(W) + 1) < 2 ** 24
    assert exact
    want = (W[-1] - np.float32(lr) * ((d_out.T @ acts[-1]).astype(np.float32) / np.float32(n))).astype(np.float32)
    assert same_bits(gW[-1], want)
    assert same_bits(loss[0], ref.loss_curve)


# ------------------------------------------------------------------ 2. the trajectory
@functools.lru_cache(maxsize=None)
def normal_data(n, d, t, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    Y = (X[:, :1] * 0.5 + rng.standard_normal((n, t))).astype(np.float32) + np.float32(1.5)
    return X, Y


def split_lists(n, seed):
    """a training list (about three quarters of the rows, shuffled) and the others as the evaluation list"""
    order = np.random.default_rng(seed).permutation(n)
    k = max(1, (3 * n) // 4)
    return order[:k], order[k:]


def scaling(X, Y):
    V = np.concatenate([X, Y], 1)
    std = V.std(0)
    return V.mean(0).astype(np.float32), np.where(std > 0, 1.0 / np.where(std > 0, std, 1.0), 1.0).astype(np.float32)


TRAJECTORIES = [(37, 5, (7,), 1, 8), (130, 48, (100,), 2, 64), (70, 17, (33, 16), 3, 32), (1, 3, (4,), 1, 200)]


@functools.lru_cache(maxsize=None)
def trajectory_ref(n, d, hidden, t, B):
    X, Y = normal_data(n, d, t, n + d)
    tr, ev = split_lists(n, 3)
    shift, scale = scaling(X, Y)
    if n == 1:
        shift, scale = None, None
    return R.fit(X, Y, hidden, tr, ev if len(ev) else None, shift=shift, scale=scale, lr=1e-2, alpha=1e-3, seed=77 + n,
                 epochs=3, batch_size=B)


@pytest.mark.parametrize("n,d,hidden,t,B", TRAJECTORIES)
def test_adam_trajectory_equals_the_restatement_bit_for_bit(n, d, hidden, t, B, dev):
    """3 epochs of Adam on seeded normal data: a short last batch (27 = 3 x 8 + 3, 97 = 64 + 33, 52 = 32 + 20) and
    B > n; weights, both moments, the beta powers, loss_curve and eval_sse"""
    X, Y = normal_data(n, d, t, n + d)
    tr, ev = split_lists(n, 3)
    shift, scale = (None, None) if n == 1 else scaling(X, Y)
    ref = trajectory_ref(n, d, hidden, t, B)
    lists, evals = ([tr, ev], [1]) if len(ev) else ([tr], [-1])
    blocks, loss, sse, info, status = run_fit(dev, X, Y, hidden, lists, [0], evals, [1e-2], [1e-3], [77 + n], shift=shift,
                                              scale=scale, epochs=3, batch_size=B)
    assert status.tolist() == [0, 0, 0, 0]
    check_model(blocks[0], loss[0], sse[0], int(info[0]), ref, d, hidden, t)
    assert ref.info == 0 and np.isfinite(ref.loss_curve).all()


# ------------------------------------------------------------------ 3. independence
def test_a_model_does_not_depend_on_its_company_strides_lists_or_cuts(dev):
    n, d, hidden, t, B = 37, 5, (7,), 1, 8
    X, Y = normal_data(n, d, t, n + d)
    tr, ev = split_lists(n, 3)
    shift, scale = scaling(X, Y)
    ref = trajectory_ref(n, d, hidden, t, B)
    kw = dict(shift=shift, scale=scale, epochs=3, batch_size=B)
    alone = run_fit(dev, X, Y, hidden, [tr, ev], [0], [1], [1e-2], [1e-3], [77 + n], **kw)
    check_model(alone[0][0], alone[1][0], alone[2][0], int(alone[3][0]), ref, d, hidden, t)
    again = run_fit(dev, X, Y, hidden, [tr, ev], [0], [1], [1e-2], [1e-3], [77 + n], **kw)
    assert all(same_bits(a, b) for a, b in zip(alone, again))                              # run to run
    # among seven others, at position 5, with other lists, rates and seeds around it; strides with NaN pads
    others = [np.arange(n), ev, tr[:9]]
    train = [2, 3, 4, 2, 0, 0, 1, 2]
    evals = [-1, 1, 1, 0, -1, 1, 0, 3]
    lrs = [1e-3, 1e-2, 3e-2, 1e-3, 1e-2, 1e-2, 1e-2, 1e-1]
    seeds = [1, 2, 3, 4, 77 + n, 77 + n, 5, 6]
    many = run_fit(dev, X, Y, hidden, [tr, ev] + others, train, evals, lrs, [1e-3] * 8, seeds, padx=3, pady=1, **kw)
    assert many[4].tolist() == [0, 0, 0, 0]
    check_model(many[0][5], many[1][5], many[2][5], int(many[3][5]), ref, d, hidden, t)
    assert (many[3] == 0).all() and not same_bits(many[0][5], many[0][6])
    # model 4 is model 5 without an evaluation list: the same state, no held-out error
    assert same_bits(many[0][4], many[0][5]) and np.isnan(many[2][4]).all() and np.isfinite(many[2][5]).all()
    # launch cuts of one epoch
    cut = run_fit(dev, X, Y, hidden, [tr, ev], [0], [1], [1e-2], [1e-3], [77 + n], cuts=1, **kw)
    assert all(same_bits(a, b) for a, b in zip(alone, cut))
    # the rows scattered in a larger array whose other rows are NaN: unlisted rows are never read
    place = np.random.default_rng(4).permutation(3 * n)[:n]
    Xs, Ys = np.full((3 * n, d), NAN, np.float32), np.full((3 * n, t), NAN, np.float32)
    Xs[place], Ys[place] = X, Y
    far = run_fit(dev, Xs, Ys, hidden, [place[tr], place[ev]], [0], [1], [1e-2], [1e-3], [77 + n], **kw)
    assert far[4].tolist() == [0, 0, 0, 0]
    assert all(same_bits(a, b) for a, b in zip(alone, far))


def test_status_reports_bad_rows_and_lists(dev):
    n, d, hidden, t = 20, 3, (4,), 1
    X, Y = normal_data(n, d, t, 1)
    X = X.copy(); X[7, 1] = NAN
    Y = Y.copy(); Y[9, 0] = np.inf
    lists = [np.arange(0, 10), np.arange(10, 20), np.array([7, 9])]
    # the list with the bad rows is used by no model: nothing is counted
    _, _, _, info, status = run_fit(dev, X, Y, hidden, lists, [1], [-1], [1e-2], [0.0], [1], epochs=1)
    assert status.tolist() == [0, 0, 0, 0] and info.tolist() == [0]
    _, _, _, info, status = run_fit(dev, X, Y, hidden, lists, [1, 1], [0, 2], [1e-2] * 2, [0.0] * 2, [1, 2], epochs=1)
    assert status.tolist() == [4, 0, 0, 0]                             # rows 7 and 9, once in list 0 and once in list 2
    _, _, _, info, status = run_fit(dev, X, Y, hidden, [np.array([3, 40, -1, 5])], [0], [-1], [1e-2], [0.0], [1], epochs=1)
    assert status[0] == 0 and status[1] == 2                           # GAE_MLP_ERR_ROW_ID: the rows are taken as zeros
    _, loss, _, info, status = run_fit(dev, X, Y, hidden, lists, [5], [-1], [1e-2], [0.0], [1], epochs=1)
    assert status[1] == 4 and info.tolist() == [-1] and np.isnan(loss).all()           # GAE_MLP_ERR_LIST_ID


def test_predict_marks_rows_with_non_finite_features(dev):
    from gae_dgl_amd import ops
    rng = np.random.default_rng(3)
    X, Y = normal_data(70, 5, 2, 9)
    res = ops.mlp(torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev), (6,), epochs=2, batch_size=16, folds=1)
    Xq = rng.standard_normal((67, 5)).astype(np.float32)
    Xq[3, 2], Xq[40, 0], Xq[66, 4] = NAN, np.inf, -np.inf
    status = torch.zeros(4, dtype=torch.int64, device=dev)
    out = as_np(res.predict(torch.from_numpy(Xq).to(dev), status=status))
    bad = np.array([3, 40, 66])
    assert np.isnan(out[bad]).all() and np.isfinite(np.delete(out, bad, 0)).all() and as_np(status).tolist() == [3, 0, 0, 0]
    W = [as_np(w)[0] for w in res.weights]
    b = [as_np(v)[0] for v in res.biases]
    want = R.predict_rows(W, b, Xq, as_np(res.shift), as_np(res.scale))
    assert same_bits(out.astype(np.float32), want) and out.dtype == np.float64


# ------------------------------------------------------------------ 4. errors
def test_errors(dev):
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    X, Y = normal_data(120, 6, 1, 2)
    Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y[:, 0].copy()).to(dev)
    bad = Xd.clone(); bad[11, 2] = NAN
    with pytest.raises(GaeHipError, match="non-finite"):
        ops.mlp(bad, yd, (8,), epochs=2, folds=3)
    fold = torch.zeros(120, dtype=torch.int64, device=dev); fold[60:] = 1; fold[11] = -1
    assert ops.mlp(bad, yd, (8,), epochs=2, folds=2, fold=fold).n_used == 119            # left out: never read
    # plain SGD at lr = 1e6 overflows within a few steps (Adam's steps are bounded by lr, its weights stay finite)
    res = ops.mlp(Xd, yd, (8,), lrs=(1e6, 1e-2), epochs=4, batch_size=32, folds=3, solver="sgd")
    info = as_np(res.info)
    assert (info[0] > 0).all() and (info[1] == 0).all() and res.lr == 1e-2
    assert np.isnan(as_np(res.cv_r2)[0]).all() and np.isfinite(as_np(res.cv_r2)[1]).all()
    with pytest.raises(GaeHipError, match="none of the 1 configurations"):
        ops.mlp(Xd, yd, (8,), lrs=(1e6,), epochs=4, batch_size=32, folds=3, solver="sgd")
    with pytest.raises(GaeHipError, match="outside 1..128"):
        ops.mlp(torch.zeros(10, 129, device=dev), torch.zeros(10, device=dev), (8,), folds=2)
    with pytest.raises(GaeHipError, match="outside 1..8"):
        ops.mlp(Xd, torch.zeros(120, 9, device=dev), (8,), folds=2)
    with pytest.raises(GaeHipError, match="LDS"):
        ops.mlp(torch.zeros(10, 128, device=dev), torch.zeros(10, device=dev), (128, 128), folds=2)
    with pytest.raises(GaeHipError):
        ops.mlp(X, yd)                                                 # a numpy array / CPU tensor: no fallback


# ------------------------------------------------------------------ 5. it learns
def test_it_learns_what_a_linear_model_cannot(dev):
    """y = |x0| - |x1| + 0.05 noise: lr = 1e-2 is chosen with cv_r2 >= 0.95, ridge on the same arrays has cv_r2 <= 0.05
    (sklearn 1.7.2's MLPRegressor with these settings: 5-fold R2 0.988-0.989 at lr = 1e-2, 0.69-0.78 at 1e-3; ridge
    -0.03 .. -0.01)"""
    from gae_dgl_amd import ops
    rng = np.random.default_rng(0)
    X = rng.standard_normal((600, 8)).astype(np.float32)
    y = (np.abs(X[:, 0]) - np.abs(X[:, 1]) + 0.05 * rng.standard_normal(600)).astype(np.float32)
    Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
    res = ops.mlp(Xd, yd, hidden=(32,), batch_size=64, epochs=60, lrs=(1e-3, 1e-2), folds=5)
    r2 = as_np(res.cv_r2)
    print(f"mlp cv_r2 at lr 1e-3 / 1e-2: {r2[0, 0]:.4f} / {r2[1, 0]:.4f}")
    assert res.lr == 1e-2 and r2[1, 0] >= 0.95
    ridge = ops.ridge(Xd, yd, folds=5)
    chosen = ridge.lambdas.tolist().index(ridge.lam)
    print(f"ridge cv_r2: {float(ridge.cv_r2[chosen, 0]):.4f}")
    assert float(ridge.cv_r2[chosen, 0]) <= 0.05
    assert (as_np(res.info) == 0).all() and res.n_used == 600 and res.fold_counts.tolist() == [120] * 5
    curve = as_np(res.loss_curve)[1, 5, 0]
    assert curve[-1] < 0.1 * curve[0]


# ------------------------------------------------------------------ 6. the surface
def mol8_dataset(dev):
    import gae_dgl_amd as G
    from conftest import load_golden
    from gae_dgl_amd.dataset import DeviceGraphDataset
    parts, whole = load_golden("mol8_parts"), load_golden("mol8")
    ng = int(parts["n_graphs"])
    sizes = [int(parts[f"g{i}/n"]) for i in range(ng)]
    gp = np.zeros(ng + 1, np.int64); np.cumsum(sizes, out=gp[1:])
    src = np.concatenate([parts[f"g{i}/src"] + gp[i] for i in range(ng)])
    dst = np.concatenate([parts[f"g{i}/dst"] + gp[i] for i in range(ng)])
    X = np.concatenate([parts[f"g{i}/X"] for i in range(ng)])
    ds = DeviceGraphDataset(gp, src, dst, X, device=dev)
    model = G.GAE(X.shape[1], [int(h) for h in whole["hidden"]])
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in whole.items() if k.startswith("sd/")})
    return ds, model.to(dev).eval(), ng


def test_mlp_graphs_is_mlp_of_the_molecule_features(dev):
    from gae_dgl_amd import ops
    ds, model, ng = mol8_dataset(dev)
    y = torch.tensor(np.random.default_rng(5).standard_normal((ng, 2)), dtype=torch.float32, device=dev)
    feats = model.embed_graphs(ds)
    kw = dict(hidden=(12, 5), lrs=(1e-2, 3e-2), epochs=5, batch_size=4, folds=2, ensemble=2, seed=9)
    want = ops.mlp(feats, y, **kw)
    res = model.mlp_graphs(ds, y, fused="auto", **kw)
    assert res.n_used == ng and res.lr == want.lr and len(res.weights) == 3 and res.weights[0].shape == (2, 12, feats.shape[1])
    for a, b in zip(list(res.weights) + list(res.biases) + [res.cv_sse, res.loss_curve, res.state],
                    list(want.weights) + list(want.biases) + [want.cv_sse, want.loss_curve, want.state]):
        assert same_bits(as_np(a), as_np(b))
    assert res.info.shape == (2, 3, 2) and res.cv_sse.shape == (2, 2, 2, 2)
    with pytest.raises(ValueError):
        model.mlp_graphs(ds, y, grad=True)


def test_to_torch_reproduces_predict(dev):
    """raw features in, raw targets out; predict is the fp64 mean of the members in member order.  Tolerance: the folded
    weights are stored in fp32 and every layer is a sum of K <= 48 products of standardised values, (K + 2) 2^-24 per
    layer and three roundings of the folding: 1e-5 of the output's size"""
    from gae_dgl_amd import ops
    X, Y = normal_data(130, 48, 2, 178)
    Xd = torch.from_numpy(X).to(dev)
    res = ops.mlp(Xd, torch.from_numpy(Y).to(dev), (20, 10), epochs=4, batch_size=32, folds=2, ensemble=3, seed=4)
    pred = as_np(res.predict(Xd))
    outs = [as_np(res.to_torch(k).to(dev)(Xd)).astype(np.float64) for k in range(3)]
    assert pred.shape == (130, 2) and pred.dtype == np.float64
    assert np.abs((outs[0] + outs[1] + outs[2]) / 3 - pred).max() <= 1e-5 * (1.0 + np.abs(pred).max())
    assert np.abs(outs[0] - outs[1]).max() > 1e-3                      # the members differ: their seeds do


def test_cli_embed_mlp_in_a_child_process(tmp_path):
    import gae_dgl_amd as G
    torch.manual_seed(0)
    ckpt = str(tmp_path / "m.pkl")
    torch.save(G.GAE(39, [32, 16]).state_dict(), ckpt)
    ng = 120
    np.save(tmp_path / "y.npy", np.random.default_rng(1).standard_normal((ng, 2)))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "gae_dgl_amd.embed", "--checkpoint", ckpt, "--hidden_dims", "32", "16",
                        "--synthetic", str(ng), "--out", str(tmp_path / "f.npy"), "--targets", str(tmp_path / "y.npy"),
                        "--mlp", "24", "--mlp_epochs", "6", "--mlp_batch", "32", "--mlp_lr", "1e-3", "1e-2", "--mlp_folds",
                        "3", "--mlp_out", str(tmp_path / "model.npz"), "--ridge", "1.0", "--ridge_folds", "3"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("MLP (24, 3-fold CV, lr = ")]
    assert len(line) == 1 and line[0].count("RMSE:") == 2 and line[0].count("R2:") == 2 and "alpha = 0.0001" in line[0], r.stdout
    assert f"Trained an MLP head on {ng} molecules, 8 models side by side" in r.stdout and "Ridge (3-fold CV" in r.stdout
    z = np.load(tmp_path / "model.npz")
    assert z["weight0"].shape == (1, 24, 48) and z["bias1"].shape == (1, 2) and z["hidden"].tolist() == [24]
    assert z["cv_r2"].shape == (2, 2) and z["shift"].shape == (50,)
    from gae_dgl_amd import ops
    net = ops.mlp_load_head(str(tmp_path / "model.npz"))
    assert net[0].in_features == 48 and net[2].out_features == 2
