"""numpy restatement of K27 (gae_mlp_fit / gae_mlp_predict, ops.mlp), written from the K27 comment of
include/gae_hip_experimental.h: every matrix product element is ONE fp32 fma chain from +0 over the summed index in
ascending order (fma32 below restates the fused multiply-add exactly), every other step is a single fp32 numpy operation
in the stated order, the Adam step size comes from fp64 beta powers, the weights from a Philox Glorot draw and the
mini-batch order from a four-round Feistel network that is cycle-walked.  The device must return the same bits.  Shared
by tests/test_mlp_cpu.py and tests/test_gpu_mlp.py."""
import collections
import math

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
ADAM, SGD = 0, 1
f32 = np.float32

Model = collections.namedtuple("Model", ["W", "b", "mW", "mb", "vW", "vb", "step", "b1p", "b2p", "loss_curve", "eval_sse",
                                         "info"])


def fma32(a, b, c):
    """fp32 fma(a, b, c) exactly: the product of two fp32 is exact in fp64, and the fp64 sum is rounded to odd (TwoSum
    tells whether it was exact), so that the rounding to fp32 afterwards is the only one that counts"""
    p, c = np.asarray(a, f32).astype(np.float64) * np.asarray(b, f32).astype(np.float64), np.asarray(c, f32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(f32)


def chain(A, B):
    """fp32 [m, n]: element (i, j) is the chain c <- fma(A[i, k], B[k, j], c) from +0 over k ascending"""
    A, B = np.asarray(A, f32), np.asarray(B, f32)
    acc = np.zeros((A.shape[0], B.shape[1]), f32)
    for k in range(A.shape[1]):
        acc = fma32(A[:, k:k + 1], B[k:k + 1, :], acc)
    return acc


def philox(ctr, draw, key):
    """philox4x32_10 of csrc/common.h over an array of counters: uint64 [4, len] holding the four 32-bit words"""
    ctr = np.asarray(ctr, np.uint64).reshape(-1)
    c = [ctr & M32, ctr >> np.uint64(32), np.full_like(ctr, draw & 0xFFFFFFFF), np.full_like(ctr, (draw >> 32) & 0xFFFFFFFF)]
    k0, k1 = key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)) & M32, p1 & M32,
             ((p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)) & M32, p0 & M32]
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c)


def layer_shapes(d, hidden, t):
    widths = [d] + list(hidden) + [t]
    return [(widths[l + 1], widths[l]) for l in range(len(widths) - 1)]           # (out, in)


def _draw(count, draw, seed, bound):
    e = np.arange(count, dtype=np.uint64)
    words = philox(e >> np.uint64(2), draw, seed)
    w = words[(e & np.uint64(3)).astype(np.int64), np.arange(count)]
    u = (w >> np.uint64(8)).astype(f32) * f32(2.0 ** -24)
    return (f32(2.0) * u - f32(1.0)) * bound


def glorot(seed, d, hidden, t):
    """(W, b): per layer fp32 [out, in] and [out]"""
    W, b = [], []
    for l, (out, inn) in enumerate(layer_shapes(d, hidden, t)):
        bound = f32(math.sqrt(6.0 / (inn + out)))
        W.append(_draw(out * inn, 2 * l, seed, bound).reshape(out, inn))
        b.append(_draw(out, 2 * l + 1, seed, bound))
    return W, b


def perm(n_train, seed, epoch, shuffle=True):
    """int64 [n_train]: the list position visited at every position of `epoch`"""
    p = np.arange(n_train, dtype=np.uint64)
    if not shuffle:
        return p.astype(np.int64)
    hb = 1
    while 4 ** hb < n_train:
        hb += 1
    mask, shift = np.uint64((1 << hb) - 1), np.uint64(hb)
    v = p.copy()
    todo = np.ones(n_train, bool)
    while todo.any():
        x = v[todo]
        hi, lo = x >> shift, x & mask
        for r in range(4):
            F = philox((np.uint64(r) << np.uint64(32)) | lo, (1 << 32) + epoch, seed)[0]
            hi, lo = lo, hi ^ (F & mask)
        x = (hi << shift) | lo
        v[todo] = x
        todo[todo] = x >= np.uint64(n_train)
    return v.astype(np.int64)


def relu(z):
    return np.where(z > 0, z, f32(0.0)).astype(f32)


def forward(W, b, Xs):
    """(activations a_0 .. a_{L-1}, yhat) of scaled rows Xs fp32 [r, d]"""
    acts, a = [], np.asarray(Xs, f32)
    for l in range(len(W)):
        acts.append(a)
        z = chain(a, W[l].T) + b[l][None, :]
        a = relu(z) if l < len(W) - 1 else z
    return acts, a


def gradients(W, b, Xs, Ys):
    """(dW chains, db chains, delta of the output) of one batch: the sums BEFORE the penalty and the division by B"""
    acts, yhat = forward(W, b, Xs)
    delta = yhat - np.asarray(Ys, f32)
    out_delta = delta
    dW, db = [None] * len(W), [None] * len(W)
    for l in range(len(W) - 1, -1, -1):
        dW[l] = chain(delta.T, acts[l])
        db[l] = chain(delta.T, np.ones((delta.shape[0], 1), f32))[:, 0]
        if l > 0:
            delta = np.where(acts[l] > 0, chain(delta, W[l]), f32(0.0)).astype(f32)
    return dW, db, out_delta


def scaled(V, shift, scale):
    return (np.asarray(V, f32) - shift[None, :]) * scale[None, :]


def fit(X, Y, hidden, train_rows, eval_rows=None, *, shift=None, scale=None, lr=1e-3, alpha=1e-4, seed=0, epochs=3,
        batch_size=200, beta1=0.9, beta2=0.999, eps=1e-8, solver=ADAM, momentum=0.0, shuffle=True, init=None, first_epoch=0):
    """`init` = (W, b): start from these weights instead of the Glorot draw (a state block written by hand), the epochs
    numbered from `first_epoch`"""
    X, Y = np.asarray(X, f32), np.asarray(Y, f32).reshape(len(X), -1)
    d, t = X.shape[1], Y.shape[1]
    shift = np.zeros(d + t, f32) if shift is None else np.asarray(shift, f32)
    scale = np.ones(d + t, f32) if scale is None else np.asarray(scale, f32)
    train_rows = np.asarray(train_rows, np.int64)
    ntr = len(train_rows)
    W, b = glorot(seed, d, hidden, t) if init is None else ([np.array(w, f32) for w in init[0]], [np.array(v, f32) for v in init[1]])
    L = len(W)
    mW, vW = [np.zeros_like(w) for w in W], [np.zeros_like(w) for w in W]
    mb, vb = [np.zeros_like(v) for v in b], [np.zeros_like(v) for v in b]
    lr, alpha, beta1, beta2, eps, momentum = f32(lr), f32(alpha), f32(beta1), f32(beta2), f32(eps), f32(momentum)
    omb1, omb2 = f32(1.0) - beta1, f32(1.0) - beta2
    step, b1p, b2p = 0, 1.0, 1.0
    loss_curve = np.full(epochs, np.nan)
    info = 0

    def rule(w, g_chain, a, m, v):
        with np.errstate(all="ignore"):
            g = (g_chain + a * w) / f32(B)
            if solver == SGD:
                vel = momentum * m - lr * g
                return w + vel, vel, v
            m2 = beta1 * m + omb1 * g
            v2 = beta2 * v + omb2 * (g * g)
            return w - step_size * (m2 / (np.sqrt(v2) / c2 + eps)), m2, v2

    for ep in range(epochs):
        order = train_rows[perm(ntr, seed, first_epoch + ep, shuffle)]
        sse, bad = 0.0, False
        for b0 in range(0, ntr, batch_size):
            ids = order[b0:b0 + batch_size]
            B = len(ids)
            with np.errstate(all="ignore"):
                dW, db, delta = gradients(W, b, scaled(X[ids], shift[:d], scale[:d]), scaled(Y[ids], shift[d:], scale[d:]))
                for e in delta.astype(np.float64).reshape(-1):
                    sse = sse + e * e
            step += 1
            b1p *= float(beta1)
            b2p *= float(beta2)
            step_size = f32(float(lr) / (1.0 - b1p))
            c2 = f32(math.sqrt(1.0 - b2p))
            for l in range(L):
                W[l], mW[l], vW[l] = rule(W[l], dW[l], alpha, mW[l], vW[l])
                b[l], mb[l], vb[l] = rule(b[l], db[l], f32(0.0), mb[l], vb[l])
                bad = bad or not (np.isfinite(W[l]).all() and np.isfinite(b[l]).all())
        loss_curve[ep] = sse / (2.0 * ntr)
        if bad or not math.isfinite(loss_curve[ep]):
            info = 1 + ep
            break
    eval_sse = np.full(t, np.nan)
    if eval_rows is not None and info == 0:
        ids = np.asarray(eval_rows, np.int64)
        back = predict_rows(W, b, X[ids], shift, scale)
        err = (back - Y[ids]).astype(np.float64)
        eval_sse = np.zeros(t)
        for i in range(len(ids)):
            eval_sse = eval_sse + err[i] * err[i]
    return Model(W, b, mW, mb, vW, vb, step, b1p, b2p, loss_curve, eval_sse, info)


def predict_rows(W, b, X, shift=None, scale=None):
    """fp32 [n, t] in the targets' own units: (yhat / scale_y) + shift_y"""
    X = np.asarray(X, f32)
    d, t = X.shape[1], W[-1].shape[0]
    shift = np.zeros(d + t, f32) if shift is None else np.asarray(shift, f32)
    scale = np.ones(d + t, f32) if scale is None else np.asarray(scale, f32)
    _, yhat = forward(W, b, scaled(X, shift[:d], scale[:d]))
    out = (yhat / scale[None, d:]) + shift[None, d:]
    out[~np.isfinite(X).all(1)] = np.nan
    return out.astype(f32)
