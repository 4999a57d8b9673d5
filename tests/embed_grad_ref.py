"""fp64 reference of the gradients of the molecule feature [mean | sum | max] (K21, gae_embed_graphs_bwd, and the
readout's own backward gae_segment_readout_bwd): torch autograd through ``oracle.gae_encode`` with ``requires_grad``
weights and a per-graph readout whose max takes the FIRST row attaining it (``tie="last"``: the last one -- the rule the
weight gradients cannot see; ``encoder_grads`` asserts that on every input it is given)."""
import numpy as np
import torch


def O():
    from oracle import gae_oracle
    return gae_oracle


def rel_err(a, b):
    """tests/test_gpu_parity.py::rel_err: max abs difference over max(1, max |reference|)"""
    a = torch.as_tensor(a).detach().double().cpu(); b = torch.as_tensor(b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    if b.numel() == 0:
        return 0.0
    return float((a - b).abs().max() / b.abs().max().clamp(min=1.0))


def readout(Z, graph_ptr, tie="first"):
    """[G, 3 d] = mean | sum | max over each graph's rows of Z (a torch tensor, differentiable); the whole gradient of a
    max goes to the first (``tie="last"``: last) row that attains it; an empty graph gives zeros"""
    gp = torch.as_tensor(np.asarray(graph_ptr, dtype=np.int64))
    G, (N, d) = len(gp) - 1, Z.shape
    sizes = gp[1:] - gp[:-1]
    gid = torch.repeat_interleave(torch.arange(G), sizes)
    s = torch.zeros(G, d, dtype=Z.dtype).index_add(0, gid, Z)
    mean = s / sizes.clamp(min=1).to(Z.dtype).unsqueeze(1)
    if N == 0:
        return torch.cat([mean, s, torch.zeros(G, d, dtype=Z.dtype)], 1)
    with torch.no_grad():
        idx = gid.unsqueeze(1).expand(N, d)
        mx = torch.full((G, d), -float("inf"), dtype=Z.dtype).scatter_reduce(0, idx, Z.detach(), "amax")
        hit = Z.detach() == mx[gid]
        rows = torch.arange(N).unsqueeze(1).expand(N, d)
        if tie == "first":
            star = torch.full((G, d), N, dtype=torch.int64).scatter_reduce(0, idx, torch.where(hit, rows, N), "amin")
        else:
            star = torch.full((G, d), -1, dtype=torch.int64).scatter_reduce(0, idx, torch.where(hit, rows, -1), "amax")
        star = star.clamp(0, N - 1)
    top = torch.where((sizes > 0).unsqueeze(1), Z.gather(0, star), torch.zeros((), dtype=Z.dtype))
    return torch.cat([mean, s, top], 1)


def readout_dz(Z, graph_ptr, d_out, tie="first"):
    """fp64 dZ [N, d] of sum(readout(Z) * d_out)"""
    Z = torch.as_tensor(np.asarray(Z)).double().requires_grad_(True)
    loss = (readout(Z, graph_ptr, tie) * torch.as_tensor(np.asarray(d_out)).double()).sum()
    return torch.autograd.grad(loss, Z)[0]


def features(gp, src, dst, X, Ws, bs, norm, graph_ids=None, tie="first"):
    """fp64 feature rows (differentiable in Ws / bs) of the graphs ``graph_ids`` (None: all, in order)"""
    n = int(gp[-1])
    ip, ix = O().csr_from_coo(src, dst, n)
    nv = O().norm_from_in_degrees(O().in_degrees(dst, n)).double() if norm == "both" else None
    Z = O().gae_encode(ip, ix, torch.as_tensor(np.asarray(X)).double(), Ws, bs, nv)
    F = readout(Z, gp, tie)
    if graph_ids is not None:
        F = F[torch.as_tensor(np.asarray(graph_ids, dtype=np.int64))]
    return F


def params_of(model):
    Ws = [l.apply_mod.linear.weight.detach().double().cpu().requires_grad_(True) for l in model.layers]
    bs = [l.apply_mod.linear.bias.detach().double().cpu().requires_grad_(True) for l in model.layers]
    return Ws, bs


def encoder_grads(gp, src, dst, X, model, norm, d_out, graph_ids=None):
    """(features, dWs, dbs) in fp64 for the loss sum(features * d_out).  PRECONDITION, asserted here for every input: the
    first-row and the last-row tie rule give the same weight gradients to 1e-9 -- an input where they do not is a bad
    input for a 1e-5 comparison, not a reason to widen it"""
    d_out = torch.as_tensor(np.asarray(d_out.detach().cpu() if isinstance(d_out, torch.Tensor) else d_out)).double()
    got = {}
    for tie in ("first", "last"):
        Ws, bs = params_of(model)
        F = features(gp, src, dst, X, Ws, bs, norm, graph_ids, tie)
        grads = torch.autograd.grad((F * d_out).sum(), Ws + bs, allow_unused=True)
        grads = [torch.zeros_like(p) if g is None else g for g, p in zip(grads, Ws + bs)]
        got[tie] = (F.detach(), grads[:len(Ws)], grads[len(Ws):])
    for a, b in zip(got["first"][1] + got["first"][2], got["last"][1] + got["last"][2]):
        assert rel_err(a, b) <= 1e-9, f"the tie rule shows in the weight gradients of this input: {rel_err(a, b):.3e}"
    return got["first"]
