"""K27 without a GPU: the numpy restatement tests/mlp_ref.py (the yardstick of tests/test_gpu_mlp.py) is checked against
fp64 torch -- its gradients within the fma-chain bound, its Adam trajectory against torch.optim.Adam -- the mini-batch
order is a permutation, and the C entry points, ops.mlp and the embed / finetune parsers reject bad arguments before any
launch."""
import ctypes

import numpy as np
import pytest
import torch

import mlp_ref as R


# ------------------------------------------------------------------ 1. the restatement itself
def test_fma32_rounds_once():
    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(4000).astype(np.float32) for _ in range(3))
    c = c * np.float32(1e-3)
    got = R.fma32(a, b, c)
    from fractions import Fraction
    for i in range(0, 4000, 97):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        assert abs(Fraction(float(got[i])) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))
    two_step = (a.astype(np.float32) * b + c).astype(np.float32)
    assert (got != two_step).any()                                     # a fused chain is not the two-step product


@pytest.mark.parametrize("n_train", [1, 2, 3, 5, 64, 200, 201, 1128])
def test_the_minibatch_order_is_a_permutation(n_train):
    p0 = R.perm(n_train, 7, 0)
    assert sorted(p0.tolist()) == list(range(n_train))
    assert R.perm(n_train, 7, 0, shuffle=False).tolist() == list(range(n_train))
    assert np.array_equal(p0, R.perm(n_train, 7, 0))
    if n_train >= 64:
        assert not np.array_equal(p0, R.perm(n_train, 7, 1))           # between epochs
        assert not np.array_equal(p0, R.perm(n_train, 8, 0))           # between seeds
        assert not np.array_equal(p0, np.arange(n_train))


def test_the_shuffle_streams_are_disjoint_from_the_init_streams():
    """the init draws use draw = 2 l and 2 l + 1 < 6, the shuffle draw = 2^32 + epoch"""
    W, b = R.glorot(3, 5, (7, 4), 2)
    assert [w.shape for w in W] == [(7, 5), (4, 7), (2, 4)] and [v.shape for v in b] == [(7,), (4,), (2,)]
    for l, w in enumerate(W):
        bound = np.float32(np.sqrt(6.0 / (w.shape[0] + w.shape[1])))
        assert np.abs(w).max() <= bound and np.abs(b[l]).max() <= bound and w.dtype == np.float32
    word = R.philox(np.array([0]), 0, 3)[0, 0]
    u = np.float32(int(word) >> 8) * np.float32(2.0 ** -24)
    assert W[0][0, 0] == (np.float32(2.0) * u - np.float32(1.0)) * np.float32(np.sqrt(6.0 / 12.0))
    assert not np.array_equal(R.glorot(4, 5, (7, 4), 2)[0][0], W[0])


def _torch_grads(W, b, Xs, Ys):
    Wt = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in W]
    bt = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in b]
    a = torch.tensor(Xs, dtype=torch.float64)
    for l in range(len(W)):
        a = a @ Wt[l].t() + bt[l]
        if l < len(W) - 1:
            a = torch.relu(a)
    loss = 0.5 * ((a - torch.tensor(Ys, dtype=torch.float64)) ** 2).sum()
    loss.backward()
    return [w.grad.numpy() for w in Wt], [v.grad.numpy() for v in bt]


@pytest.mark.parametrize("n,d,hidden,t", [(37, 5, (7,), 1), (70, 17, (33, 16), 3)])
def test_gradients_against_fp64_autograd_within_the_chain_bound(n, d, hidden, t):
    """dW of the output layer is ONE chain of K = n terms on an operand that is itself within a forward chain's bound of
    the fp64 value; the bound 2 (K + 2) 2^-24 sum |a b| is taken per element with K the longest chain on the way to
    that element (the batch rows plus the widest layer), sum |a b| from the fp64 operands"""
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, d)).astype(np.float32)
    Y = rng.standard_normal((n, t)).astype(np.float32)
    W, b = R.glorot(11, d, hidden, t)
    dW, db, delta = R.gradients(W, b, X, Y)
    gW, gb = _torch_grads(W, b, X, Y)
    # fp64 magnitudes: |delta|^T |a| per layer with the fp64 forward and |W| in the backward
    acts, a = [], X.astype(np.float64)
    for l in range(len(W)):
        acts.append(a)
        a = a @ W[l].astype(np.float64).T + b[l]
        if l < len(W) - 1:
            a = np.maximum(a, 0)
    mag = np.abs(a - Y)
    for l in range(len(W) - 1, -1, -1):
        K = n + max([d] + list(hidden))
        bound = 2 * (K + 2) * 2.0 ** -24
        slack_W = bound * (mag.T @ np.abs(acts[l])) + 1e-30
        slack_b = bound * mag.sum(0) + 1e-30
        assert (np.abs(dW[l] - gW[l]) <= slack_W).all(), (l, np.abs(dW[l] - gW[l]).max(), slack_W.min())
        assert (np.abs(db[l] - gb[l]) <= slack_b).all(), l
        mag = (mag @ np.abs(W[l].astype(np.float64))) + bound * 0
    assert delta.shape == (n, t)


def test_adam_trajectory_against_torch_adam():
    """10 Adam steps (one batch per epoch, alpha = 0, no shuffle) against torch.optim.Adam in fp64 on the same start.
    Measured on the CPU: the largest weight deviation after 10 steps is 1.364e-07 at weights of order 0.5 and lr = 1e-2
    (fp32 rounding of the weights, moments and gradients; every step moves a weight by about lr); the assertion is that
    value with a factor 4 of margin."""
    n, d, hidden, t = 37, 5, (7,), 1
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, d)).astype(np.float32)
    Y = rng.standard_normal((n, t)).astype(np.float32)
    seed, lr = 21, 1e-2
    m = R.fit(X, Y, hidden, np.arange(n), lr=lr, alpha=0.0, seed=seed, epochs=10, batch_size=n, shuffle=False)
    assert m.info == 0 and m.step == 10
    W0, b0 = R.glorot(seed, d, hidden, t)
    params = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for pair in zip(W0, b0) for v in pair]
    opt = torch.optim.Adam(params, lr=float(np.float32(lr)), betas=(float(np.float32(0.9)), float(np.float32(0.999))),
                           eps=float(np.float32(1e-8)))
    Xt, Yt = torch.tensor(X, dtype=torch.float64), torch.tensor(Y, dtype=torch.float64)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        h = torch.relu(Xt @ params[0].t() + params[1])
        out = h @ params[2].t() + params[3]
        loss = 0.5 * ((out - Yt) ** 2).sum() / n
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    dev = max(float(np.abs(w - p.detach().numpy()).max()) for w, p in zip([m.W[0], m.b[0], m.W[1], m.b[1]], params))
    print(f"Adam, 10 steps: largest deviation from torch.optim.Adam in fp64 {dev:.3e}")
    assert dev <= 4 * 1.364e-07
    assert np.allclose(m.loss_curve, losses, rtol=1e-5)
    assert m.loss_curve[-1] < m.loss_curve[0]


def test_batches_and_loss_bookkeeping():
    """a short last batch, B > n as one batch, the loss as the epoch's SSE / (2 n_train), eval in the targets' units"""
    rng = np.random.default_rng(9)
    X = rng.standard_normal((21, 3)).astype(np.float32)
    Y = (3.0 + 2.0 * rng.standard_normal((21, 2))).astype(np.float32)
    shift = np.concatenate([X.mean(0), Y.mean(0)]).astype(np.float32)
    scale = (1.0 / np.concatenate([X.std(0), Y.std(0)])).astype(np.float32)
    a = R.fit(X, Y, (4,), np.arange(16), np.arange(16, 21), shift=shift, scale=scale, epochs=2, batch_size=5, seed=1)
    assert a.step == 2 * 4 and a.info == 0 and np.isfinite(a.loss_curve).all()
    b = R.fit(X, Y, (4,), np.arange(16), epochs=2, batch_size=200, seed=1)
    assert b.step == 2 and np.isnan(b.eval_sse).all()
    back = R.predict_rows(a.W, a.b, X[16:], shift, scale)
    assert np.allclose(a.eval_sse, ((back - Y[16:]).astype(np.float64) ** 2).sum(0), rtol=1e-12)
    X2 = X.copy(); X2[17, 1] = np.inf
    assert np.isnan(R.predict_rows(a.W, a.b, X2[16:], shift, scale)[1]).all()
    c = R.fit(X, Y, (4,), np.arange(16), epochs=3, batch_size=8, lr=1e6, solver=R.SGD, seed=1)
    assert c.info >= 1 and np.isnan(c.loss_curve[c.info:]).all()


# ------------------------------------------------------------------ 2. argument handling
def test_the_workspace_query_states_limits_and_fit():
    from gae_dgl_amd import _lib, ops
    lib = _lib.load()
    q = lib.gae_mlp_workspace_bytes
    for d, h1, h2, t in [(48, 100, 0, 1), (48, 64, 64, 1), (128, 128, 0, 8), (1, 1, 0, 1), (128, 64, 128, 8)]:
        one = q(d, h1, h2, t, 1)
        assert one > 0 and one % 256 == 0 and q(d, h1, h2, t, 7) == 7 * one and q(d, h1, h2, t, 4096) == 4096 * one
        params = d * h1 + h1 + (h1 * h2 + h2 + h2 * t + t if h2 else h1 * t + t)
        assert one >= 4 * (_lib.MLP_STATE_HEADER + 3 * params)
        assert ops.mlp_usable(d, (h1, h2) if h2 else (h1,), t)
    for bad in [(0, 4, 0, 1, 1), (129, 4, 0, 1, 1), (4, 0, 0, 1, 1), (4, 129, 0, 1, 1), (4, 4, 129, 1, 1), (4, 4, -1, 1, 1),
                (4, 4, 0, 0, 1), (4, 4, 0, 9, 1), (4, 4, 0, 1, 0), (4, 4, 0, 1, 4097)]:
        assert q(*bad) == -6 and b"gae_mlp_workspace_bytes" in lib.gae_last_error(), bad
    assert q(128, 128, 128, 8, 1) == -6 and b"LDS" in lib.gae_last_error()        # inside the limits, too large on chip
    assert not ops.mlp_usable(128, (128, 128), 8) and not ops.mlp_usable(4, (4, 4, 4), 1) and not ops.mlp_usable(4, (), 1)
    assert not ops.mlp_usable(200, (4,), 1) and ops.mlp_usable(4, 4, 1)


def test_fit_and_predict_argument_errors_do_not_need_a_gpu():
    from gae_dgl_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(256)                                         # a non-NULL address that is never dereferenced
    f = ctypes.c_float

    def fit(**kw):
        a = dict(X=one, ldx=4, Y=one, ldy=1, n=10, d=4, h1=8, h2=0, t=1, shift=None, scale=None, rows=one, n_rows=10,
                 list_ptr=one, n_lists=1, train=one, eval=one, lr=one, alpha=one, seed=one, M=1, B=4, b1=0.9, b2=0.999,
                 eps=1e-8, solver=0, mom=0.0, flags=0, e0=0, e1=1, epochs=1, loss=one, sse=one, info=one, status=one,
                 ws=one, ws_bytes=1 << 20)
        a.update(kw)
        return lib.gae_mlp_fit(a["X"], a["ldx"], a["Y"], a["ldy"], a["n"], a["d"], a["h1"], a["h2"], a["t"], a["shift"],
                               a["scale"], a["rows"], a["n_rows"], a["list_ptr"], a["n_lists"], a["train"], a["eval"],
                               a["lr"], a["alpha"], a["seed"], a["M"], a["B"], f(a["b1"]), f(a["b2"]), f(a["eps"]),
                               a["solver"], f(a["mom"]), a["flags"], a["e0"], a["e1"], a["epochs"], a["loss"], a["sse"],
                               a["info"], a["status"], a["ws"], a["ws_bytes"], None)
    RANGE, SIZE, NULL, WORKSPACE = -6, -2, -1, -5
    for kw, rc in [(dict(d=0), RANGE), (dict(h1=200), RANGE), (dict(t=9), RANGE), (dict(M=5000), RANGE), (dict(B=0), RANGE),
                   (dict(n_lists=0), RANGE), (dict(n_lists=2000), RANGE), (dict(solver=2), RANGE), (dict(flags=4), RANGE),
                   (dict(b1=1.0), RANGE), (dict(eps=0.0), RANGE), (dict(mom=1.5), RANGE), (dict(e0=1, e1=1), RANGE),
                   (dict(e1=2), RANGE), (dict(epochs=0), RANGE), (dict(h1=128, h2=128, d=128), RANGE),
                   (dict(ldx=3), SIZE), (dict(ldy=0), SIZE), (dict(n=-1), SIZE), (dict(n_rows=0), SIZE),
                   (dict(n_rows=1 << 31), SIZE), (dict(X=None), NULL), (dict(rows=None), NULL), (dict(seed=None), NULL),
                   (dict(loss=None), NULL), (dict(status=None), NULL), (dict(ws=None), NULL), (dict(ws_bytes=16), WORKSPACE)]:
        assert fit(**kw) == rc, (kw, lib.gae_last_error())
        assert b"gae_mlp_fit" in lib.gae_last_error()

    def predict(X=one, ldx=4, n=10, d=4, h1=8, h2=0, t=1, state=one, M=1, out=one):
        return lib.gae_mlp_predict(X, ldx, n, d, h1, h2, t, None, None, state, M, out, None, None)
    for kw, rc in [(dict(d=129), RANGE), (dict(t=0), RANGE), (dict(M=0), RANGE), (dict(ldx=3), SIZE), (dict(n=-1), SIZE),
                   (dict(state=None), NULL), (dict(X=None), NULL), (dict(out=None), NULL)]:
        assert predict(**kw) == rc, (kw, lib.gae_last_error())
    assert predict(n=0, X=None, out=None) == 0                         # nothing to do, nothing launched


def test_ops_mlp_option_errors():
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    X, y = torch.zeros(10, 4), torch.zeros(10)
    for kw in [dict(hidden=()), dict(hidden=(4, 4, 4)), dict(hidden=(0,)), dict(hidden=(129,)), dict(hidden=(4.5,)),
               dict(lrs=()), dict(lrs=(0.0,)), dict(lrs=(float("nan"),)), dict(alphas=(-1.0,)), dict(epochs=0),
               dict(epochs=1.5), dict(batch_size=0), dict(folds=0), dict(folds=33), dict(folds=True), dict(ensemble=0),
               dict(folds=1, lrs=(1e-3, 1e-2)), dict(folds=32, lrs=[1e-3] * 10, alphas=[0.0] * 13), dict(seed=-1),
               dict(solver="lbfgs"), dict(momentum=1.0), dict(momentum=0.5), dict(shuffle=1), dict(standardize=None)]:
        with pytest.raises(ValueError):
            ops.mlp(X, y, **kw)
    with pytest.raises(GaeHipError):                                   # options are fine: a CPU tensor has no fallback
        ops.mlp(X, y)
    seeds = {ops.mlp.__globals__["model_seed"](5, c, f, k) for c in range(3) for f in range(4) for k in range(2)}
    assert len(seeds) == 24 and all(0 <= s < 2 ** 64 for s in seeds)
    assert ops.mlp.__globals__["model_seed"](5, 1, 2, 0) != ops.mlp.__globals__["model_seed"](6, 1, 2, 0)


BASE = ["--checkpoint", "m.pkl", "--hidden_dims", "32", "16", "--synthetic", "10", "--out", "f.npy"]


@pytest.mark.parametrize("extra,message", [
    (["--mlp"], "--mlp needs --targets"),
    (["--mlp_epochs", "5"], "need --mlp"),
    (["--mlp_out", "m.npz"], "need --mlp"),
    (["--mlp_lr", "0.1"], "need --mlp"),
    (["--mlp", "4", "4", "4", "--targets", "y.npy"], "one or two hidden widths"),
    (["--mlp", "200", "--targets", "y.npy"], "one or two hidden widths"),
    (["--mlp", "--targets", "y.npy", "--mlp_folds", "1"], "--mlp_folds 1"),
    (["--mlp", "--targets", "y.npy", "--mlp_epochs", "0"], "positive numbers"),
    (["--mlp", "--targets", "y.npy", "--mlp_lr", "-1"], "--mlp_lr takes finite values > 0"),
    (["--mlp", "--targets", "y.npy", "--mlp_ensemble", "1000"], "models, at most"),
    (["--mlp", "--targets", "/no/such/y.npy"], "no such file"),
])
def test_the_embed_parser_refuses_impossible_mlp_combinations(extra, message, capsys):
    from gae_dgl_amd import embed
    with pytest.raises(SystemExit):
        embed.parse_args(BASE + extra)
    assert message in capsys.readouterr().err


def test_the_embed_parser_takes_mlp_beside_the_other_heads(tmp_path):
    from gae_dgl_amd import embed, finetune
    y = tmp_path / "y.npy"
    np.save(y, np.zeros(10))
    args = embed.parse_args(BASE + ["--targets", str(y), "--mlp", "64", "32", "--mlp_lr", "1e-3", "1e-2", "--ridge",
                                    "--forest", "8", "--neighbours", "3"])
    assert args.mlp == [64, 32] and args.mlp_lr == [1e-3, 1e-2] and args.ridge == [] and args.forest == 8
    assert embed.parse_args(BASE + ["--targets", str(y), "--mlp"]).mlp == []
    wide = ["--checkpoint", "m.pkl", "--hidden_dims", "64", "48", "--synthetic", "10", "--out", "f.npy"]
    with pytest.raises(SystemExit):
        embed.parse_args(wide + ["--targets", str(y), "--mlp"])        # 3 d = 144 > 128
    ft = ["--checkpoint", "m.pkl", "--hidden_dims", "32", "16", "--synthetic", "10", "--targets", str(y), "--out", "o"]
    assert finetune.parse_args(ft).head_init is None
    with pytest.raises(SystemExit):
        finetune.parse_args(ft + ["--head_init", str(y)])              # needs --head mlp
    with pytest.raises(SystemExit):
        finetune.parse_args(ft + ["--head", "mlp", "--head_init", "/no/such.npz"])
    assert finetune.parse_args(ft + ["--head", "mlp", "--head_init", str(y)]).head_init == str(y)


def test_to_torch_folds_the_scaling(tmp_path):
    """MLPResult.to_torch / ops.mlp_load_head on host tensors: raw features in, raw targets out"""
    from gae_dgl_amd import ops
    rng = np.random.default_rng(2)
    d, h, t, E = 5, 6, 2, 2
    Ws = [torch.tensor(rng.standard_normal((E, h, d)), dtype=torch.float32),
          torch.tensor(rng.standard_normal((E, t, h)), dtype=torch.float32)]
    bs = [torch.tensor(rng.standard_normal((E, h)), dtype=torch.float32), torch.tensor(rng.standard_normal((E, t)), dtype=torch.float32)]
    shift = torch.tensor(rng.standard_normal(d + t), dtype=torch.float32)
    scale = torch.tensor(0.5 + rng.random(d + t), dtype=torch.float32)
    res = ops.MLPResult(Ws, bs, 1e-3, 0.0, [1e-3], [0.0], None, None, None, None, None, 10, None, shift, scale, (h,), None)
    X = torch.tensor(rng.standard_normal((9, d)), dtype=torch.float64)
    for k in range(E):
        net = res.to_torch(k).double()
        a = torch.relu(((X - shift[:d]) * scale[:d]) @ Ws[0][k].double().t() + bs[0][k].double())
        want = (a @ Ws[1][k].double().t() + bs[1][k].double()) / scale[d:] + shift[d:]
        assert torch.allclose(net(X), want, rtol=1e-5, atol=1e-5)
    np.savez(tmp_path / "m.npz", hidden=np.array([h]), shift=shift.numpy(), scale=scale.numpy(), weight0=Ws[0].numpy(),
             bias0=bs[0].numpy(), weight1=Ws[1].numpy(), bias1=bs[1].numpy())
    net = ops.mlp_load_head(str(tmp_path / "m.npz"), member=1)
    assert torch.equal(net[0].weight, res.to_torch(1)[0].weight) and torch.equal(net[2].bias, res.to_torch(1)[2].bias)
