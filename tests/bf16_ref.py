"""bf16 rounding contract of the bf16-stored kernels, restated in numpy (fp64 in, bf16 out).

The SpMM kernels accumulate in fp32 and store every output element with ONE round-to-nearest-even rounding to bf16
(common.h f32_to_bf16).  Two ways to hold them to it:
  * exact inputs -- H of small integers times a power of two, power-of-two scales: every fp32 partial sum is exact in
    any order, so the output must equal rne_bf16(fp64 sum) bit for bit, ties included;
  * any inputs -- the fp32 sum lies within delta of the fp64 sum (fp32_sum_bound), and rounding is monotone, so the
    output must lie in bf16_bracket(ref, delta) = [rne(ref - delta), rne(ref + delta)], element by element.

Shared by tests/test_bf16_ref_cpu.py and the bf16 GPU tests."""
import warnings

import numpy as np
import torch

U32 = 2.0 ** -24                      # unit roundoff of fp32
BF16_MAX = (2.0 - 2.0 ** -7) * 2.0 ** 127
BF16_MIN_NORMAL = 2.0 ** -126
BF16_MIN_SUB = 2.0 ** -133


def rne_bf16(x64):
    """float64 -> the nearest bf16 value (round to nearest, ties to even), rounded ONCE, as float64.

    Quantum of |x| in [2^e, 2^(e+1)): 2^(e-7), from e = -126 down to the subnormal spacing 2^-133.  x / quantum is
    exact in fp64 and np.rint rounds half to even, so this is the bf16 rounding of the fp64 value itself -- not of its
    fp32 rounding (which can round twice).  Beyond the largest finite bf16 (ties included: the even neighbour of
    0x7F7F is 2^128) the result is +-Inf; the sign of zero is kept; NaN stays NaN."""
    x = np.asarray(x64, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        _, e = np.frexp(x)                                       # |x| in [2^(e-1), 2^e)
        q = np.ldexp(1.0, np.maximum(e - 1, -126) - 7)
        y = np.rint(x / q) * q
        y = np.where(np.abs(y) > BF16_MAX, np.copysign(np.inf, x), y)
    return np.where(np.isfinite(x), y, x)


def bf16_bits(x64):
    """uint16 bit patterns of rne_bf16(x64).  NaN: sign and the top 7 payload bits of the fp64 NaN, quiet bit set (what
    f32_to_bf16 does to an fp32 NaN: (u >> 16) | 0x40)."""
    x = np.asarray(x64, dtype=np.float64)
    y = rne_bf16(x)
    with np.errstate(over="ignore", invalid="ignore"):
        bits = (y.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    u = x.view(np.uint64)
    nan = ((u >> np.uint64(63)) << np.uint64(15)) | np.uint64(0x7F80) | ((u >> np.uint64(45)) & np.uint64(0x7F)) \
        | np.uint64(0x40)
    return np.where(np.isnan(x), nan.astype(np.uint16), bits)


def from_bits(bits):
    """bf16 bit patterns -> float64"""
    b = np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)
    return b.view(np.float32).astype(np.float64)


def tensor_bits(t):
    """uint16 bit patterns of a bf16 torch tensor (any device)"""
    assert t.dtype == torch.bfloat16
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def fp32_sum_bound(abs_sum, k, c=4.0):
    """delta = c k 2^-24 sum|terms| (+ k 2^-149 for fp32 subnormal steps): how far an fp32 evaluation of a k-term sum,
    in ANY order, can lie from its exact value.  Recursive or tree summation of k terms: gamma_(k-1) sum|t|
    (Higham, Accuracy and Stability of Numerical Algorithms, 4.2); the scale products enter fused (fmaf: one rounding per
    term, gamma_k), the row-scale multiply and the GAE_SPMM_ACCUMULATE addition of the old value add one rounding each:
    gamma_(k+2) <= 1.01 (k + 2) u <= 4 k u for every k >= 1 (k u < 1e-3).  c = 4 therefore covers every launch form of
    gae_spmm_csr; sum|terms| counts |rs cs h| of each edge and |old|."""
    k = np.maximum(np.asarray(k, dtype=np.float64), 1.0)
    return c * k * U32 * np.asarray(abs_sum, dtype=np.float64) + k * 2.0 ** -149


def bf16_bracket(ref64, err_bound):
    """(lo, hi) bf16 values, as float64: an fp32 result within err_bound of ref64, rounded once to bf16, lies in
    [lo, hi] (rounding is monotone).  Elementwise; NaN where ref64 is NaN."""
    ref = np.asarray(ref64, dtype=np.float64)
    d = np.asarray(err_bound, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return rne_bf16(ref - d), rne_bf16(ref + d)


def spmm64(indptr, indices, H, row_scale=None, col_scale=None, old=None):
    """(ref, abs_sum, k) of M = diag(rs) A diag(cs) H (+ old) in fp64: the exact value (to fp64 rounding), the sum of
    the absolute values of its terms, and the number of terms per row (edges, + 1 with ``old``)"""
    ip = torch.as_tensor(np.asarray(indptr, dtype=np.int64))
    ix = torch.as_tensor(np.asarray(indices, dtype=np.int64))
    H = torch.as_tensor(np.asarray(H, dtype=np.float64))
    n = ip.numel() - 1
    vals = torch.ones(ix.numel(), dtype=torch.float64)
    if col_scale is not None:
        vals = torch.as_tensor(np.asarray(col_scale, dtype=np.float64)).reshape(-1)[ix]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                              # (sparse CSR: "beta" notice)
        A = torch.sparse_csr_tensor(ip, ix, vals, size=(n, H.shape[0]), dtype=torch.float64)
        ref = (A @ H).numpy() if ix.numel() else np.zeros((n, H.shape[1]))
        asum = (torch.sparse_csr_tensor(ip, ix, vals.abs(), size=(n, H.shape[0]), dtype=torch.float64) @ H.abs()).numpy() \
            if ix.numel() else np.zeros((n, H.shape[1]))
    if row_scale is not None:
        rs = np.asarray(row_scale, dtype=np.float64).reshape(-1, 1)
        ref, asum = ref * rs, asum * np.abs(rs)
    k = np.diff(np.asarray(indptr, dtype=np.int64)).reshape(-1, 1).astype(np.float64)
    if old is not None:
        old = np.asarray(old, dtype=np.float64)
        ref, asum, k = ref + old, asum + np.abs(old), k + 1
    return ref, asum, np.broadcast_to(k, ref.shape)


def assert_in_bracket(out_bits, ref64, err_bound, what="", bracket=None):
    """every element of the bf16 output (bit patterns) lies in its bracket (``bracket``: precomputed (lo, hi)); NaN
    exactly where ref64 is NaN"""
    out = from_bits(out_bits)
    ref = np.asarray(ref64, dtype=np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(out), nan), (what, "NaN pattern", np.argwhere(np.isnan(out) != nan)[:5])
    lo, hi = bf16_bracket(ref, err_bound) if bracket is None else bracket
    with np.errstate(invalid="ignore"):
        bad = ~nan & ~((out >= lo) & (out <= hi))
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside their bf16 bracket, first at {i}: "
                             f"got {out[i]!r}, bracket [{lo[i]!r}, {hi[i]!r}], fp64 {ref[i]!r}")


def assert_spmm_bf16(out, indptr, indices, H, row_scale=None, col_scale=None, old=None, what=""):
    """a bf16-stored gae_spmm_csr result (``old``: the values GAE_SPMM_ACCUMULATE added to) against its fp64 value:
    every element in its bf16 bracket -- an elementwise check, whatever the launch form's summation order"""
    np64 = lambda t: None if t is None else torch.as_tensor(t).detach().cpu().double().numpy()
    ip = torch.as_tensor(indptr).cpu().numpy().astype(np.int64)
    ix = torch.as_tensor(indices).cpu().numpy().astype(np.int64)
    ref, asum, k = spmm64(ip, ix, np64(H), np64(row_scale), np64(col_scale), np64(old))
    assert_in_bracket(tensor_bits(out), ref, fp32_sum_bound(asum, k), what)


# ---------------------------------------------------------------- the bf16 VGAE step (BASELINE config 5) against fp64
def nerr(a, b):
    """max |a - b| normalised by the scale of b itself (max |b|): no floor of 1, which would turn a small tensor --
    a gradient well below 1 -- into an absolute test"""
    a = torch.as_tensor(a).detach().double().cpu(); b = torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max())


def vgae_step64(src, dst, n, X, params, eps, M=None):
    """the VGAE step (shared ReLU GCN layer, identity mu / log-sigma heads, z = mu + eps exp(log sigma), weighted BCE +
    KL, gradients of every parameter) in fp64 from the SAME inputs the device used: X (the bf16-stored values), the
    fp32 parameters, the device's noise.  ``M``: the layer-1 aggregate as the device stored it (the reference order
    rounds A X to bf16 before the Linear); None: A X exact (the transform-first order never stores it)."""
    from oracle import gae_oracle as O
    ip, ix = O.csr_from_coo(src, dst, n)
    Q = {k: torch.tensor(np.asarray(torch.as_tensor(v).detach().cpu().double()), dtype=torch.float64,
                         requires_grad=True) for k, v in params.items()}
    W1, b1 = Q["shared.apply_mod.linear.weight"], Q["shared.apply_mod.linear.bias"]
    if M is None:
        h = O.gcn_layer(ip, ix, torch.as_tensor(np.asarray(X, dtype=np.float64)), W1, b1, "relu")
    else:
        h = torch.relu(torch.as_tensor(np.asarray(M, dtype=np.float64)) @ W1.t() + b1)
    mu = O.gcn_layer(ip, ix, h, Q["mu_head.apply_mod.linear.weight"], Q["mu_head.apply_mod.linear.bias"], "identity")
    ls = O.gcn_layer(ip, ix, h, Q["logstd_head.apply_mod.linear.weight"], Q["logstd_head.apply_mod.linear.bias"],
                     "identity")
    z = mu + torch.as_tensor(eps).detach().cpu().double() * torch.exp(ls)
    adj = O.dense_adjacency(src, dst, n, dtype=torch.float64)
    rec = O.bce_with_logits_mean(z @ z.t(), adj, O.pos_weight_of(adj))
    kl = O.vgae_kl(mu, ls)
    loss = rec + kl
    loss.backward()
    out = {"mu": mu.detach(), "logstd": ls.detach(), "z": z.detach(), "rec": rec.detach(), "kl": kl.detach(),
           "loss": loss.detach()}
    out.update({"grad " + k: q.grad for k, q in Q.items()})
    return out


def vgae_bf16_errors(src, dst, n, X, seed=11, orders=("transform", "reference"), fused_heads=(True, False)):
    """run the VGAE step on bf16-stored X (cuda:0) in both layer-1 orders -- "transform": act(A (X W^T) + b) through
    gae_xw_fwd, "reference": the bf16 aggregate M = A X, float_rows, the fp32 Linear -- with the fused mu / log-sigma
    heads on and off, and return {(order, fused): {tensor: nerr against vgae_step64}}.  In the reference order the
    oracle takes the device's own M, after checking every element of it against its bf16 bracket (fp32 and fp64 sums
    may fall on opposite sides of a rounding boundary)."""
    import gae_dgl_amd as G
    from gae_dgl_amd import gae as gae_mod, ops, vgae as V
    dev = "cuda:0"
    torch.manual_seed(0)
    model = V.VGAE(X.shape[1], [32, 16], seed=seed).to(dev)
    g = G.DGLGraph((src, dst), num_nodes=n).to(dev)
    Xd = ops.pad_rows(torch.from_numpy(X).to(dev).to(torch.bfloat16))     # rows of whole 128-byte lines, as bench.py
    X64 = Xd.double().cpu().numpy()
    params = {k: p.detach().cpu().clone() for k, p in model.named_parameters()}
    ip, ix = g.csr()
    refs, errs = {}, {}
    for order in orders:
        for fused in fused_heads:
            model.zero_grad(set_to_none=True)
            model._draws, model.last = None, {}
            seen = []
            orig = (ops.float_rows, gae_mod.TRANSFORM_FIRST_AUTO, V.FUSE_HEADS)
            ops.float_rows = lambda t, f=orig[0]: (seen.append(t.detach().clone()), f(t))[1]
            gae_mod.TRANSFORM_FIRST_AUTO, V.FUSE_HEADS = order == "transform", fused
            xw0 = ops.STATS["xw_fwd"]
            try:
                g.ndata['h'] = Xd
                loss = model.loss(g)
                loss.backward()
            finally:
                ops.float_rows, gae_mod.TRANSFORM_FIRST_AUTO, V.FUSE_HEADS = orig
            torch.cuda.synchronize()
            if order == "transform":
                assert ops.STATS["xw_fwd"] > xw0 and not seen, "layer 1 did not run through gae_xw_fwd"
                M = None
            else:
                assert ops.STATS["xw_fwd"] == xw0 and len(seen) == 1 and seen[0].dtype == torch.bfloat16
                M = seen[0]
                assert_spmm_bf16(M, ip, ix, Xd, what="layer-1 aggregate M")
            eps = model.last["eps"].detach().cpu()
            key = (order, eps.numpy().tobytes())
            if key not in refs:
                refs[key] = (M, vgae_step64(src, dst, n, X64, params, eps, None if M is None else M.double().cpu()))
            assert M is None or torch.equal(M, refs[key][0])
            ref = refs[key][1]
            got = {k: model.last[k] for k in ("mu", "logstd", "z", "rec", "kl")}
            got["loss"] = loss
            got.update({"grad " + k: p.grad for k, p in model.named_parameters()})
            errs[(order, fused)] = {k: nerr(got[k], ref[k]) for k in ref}
    return errs


def assert_vgae_errors(errs, tol, what=""):
    worst = {key: max(e.items(), key=lambda kv: kv[1]) for key, e in errs.items()}
    print(f"\nVGAE bf16 {what}: worst normalised error per run {worst}")
    for key, e in errs.items():
        bad = {k: v for k, v in e.items() if not v < tol}
        assert not bad, (what, key, bad)
