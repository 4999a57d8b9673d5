"""The molecule feature of a whole resident set in one launch (K19, gae_embed_graphs): for every selected member graph
the complete GCN encoder on that graph's own rows followed by the [mean | sum | max] readout -- the node embeddings
never reach memory.  ``GAE.embed_graphs`` is the model-level entry; ``python -m gae_dgl_amd.embed`` the script.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import ctypes

import torch

import gae_dgl_amd.ops as _ops
from .. import _lib
from .._lib import GaeHipError
from ._base import _gpu, _on_device, _ptr, _stream, _ws_bytes

__all__ = ['EMBED_MAX_LAYERS', 'EMBED_MAX_WIDTH', 'EMBED_MAX_NODES', 'embed_graphs_usable', 'embed_graphs',
           'embed_graphs_bwd_usable', 'embed_graphs_bwd']

EMBED_MAX_LAYERS, EMBED_MAX_WIDTH, EMBED_MAX_NODES = 4, 64, 64      # the shapes gae_embed_graphs takes

_NORMS = {"none": _lib.EMBED_NORM_NONE, "both": _lib.EMBED_NORM_BOTH}


def embed_graphs_usable(f_in, widths, max_graph_nodes=0):
    """does gae_embed_graphs take an encoder ``f_in -> widths[0] -> ...`` on graphs of at most ``max_graph_nodes`` nodes?
    (1..4 layers, every width and f_in in 1..64, at most 64 nodes per graph).  Asks the library; no launch, no GPU."""
    widths = [int(w) for w in widths]
    arr = (ctypes.c_int64 * max(len(widths), 1))(*widths)
    return bool(_lib.load().gae_embed_graphs_usable(int(f_in), len(widths), arr, int(max_graph_nodes)))


def _feature_rows(feat, who="embed_graphs"):
    """(tensor that owns the rows, dtype code, elements between rows, data columns) of a feature matrix whose rows are
    whole 16-byte vectors on 16-byte boundaries; a matrix laid out otherwise is copied into such rows once"""
    if feat.dim() != 2:
        raise GaeHipError(f"{who}: feat must be [N, F], got {tuple(feat.shape)}")
    if feat.dtype == torch.uint8:
        code, q = _lib.U8, 16
    elif feat.dtype == torch.float32:
        code, q = _lib.F32, 4
    else:
        raise GaeHipError(f"{who}: uint8 or fp32 features expected, got {feat.dtype}")
    n, f = feat.shape
    need = (f + q - 1) // q * q
    ok = (f == 0 or feat.stride(1) == 1) and (n <= 1 or (feat.stride(0) % q == 0 and feat.stride(0) >= need)) \
        and feat.data_ptr() % 16 == 0
    if ok and n == 1:                       # a single row: its storage must still hold whole vectors
        ok = feat.untyped_storage().nbytes() - feat.storage_offset() * feat.element_size() >= need * feat.element_size()
    if ok and n > 1:
        return feat, code, feat.stride(0), f
    if ok and n <= 1:
        return feat, code, need, f
    buf = torch.zeros(n, need, dtype=feat.dtype, device=feat.device)
    buf[:, :f] = feat
    return buf, code, need, f


def _request(who, graph_ptr, indptr, indices, feat, weights, biases, acts, norm, graph_ids, max_graph_nodes):
    """the checked arguments gae_embed_graphs and gae_score_graphs share: (leading C arguments up to n_out, tensors to
    keep alive, device, B, widths, N, dtype code)"""
    graph_ptr = _gpu(graph_ptr, "graph_ptr")
    dev = graph_ptr.device
    for name, t in (("indptr", indptr), ("indices", indices), ("feat", feat)):
        if _gpu(t, name).device != dev:
            raise GaeHipError(f"{who}: {name} is on {t.device}, graph_ptr on {dev}")
    if graph_ptr.dtype != torch.int64 or graph_ptr.dim() != 1 or graph_ptr.numel() < 1:
        raise GaeHipError(f"{who}: graph_ptr must be an int64 [G + 1] tensor")
    if indptr.dtype != torch.int32 or indices.dtype != torch.int32:
        raise GaeHipError(f"{who}: indptr / indices must be int32 (the CSR of the resident set)")
    if norm not in _NORMS:
        raise GaeHipError(f"{who}: norm must be 'none' or 'both', got {norm!r}")
    weights, acts = list(weights), [int(a) for a in acts]
    biases = [None] * len(weights) if biases is None else list(biases)
    if not (len(weights) == len(biases) == len(acts)):
        raise GaeHipError(f"{who}: weights, biases and acts must list the same layers")
    graph_ptr, indptr, indices = graph_ptr.contiguous(), indptr.contiguous(), indices.contiguous()
    G = graph_ptr.numel() - 1
    N = indptr.numel() - 1
    rows, code, ldf, f_in = _feature_rows(feat.detach(), who)
    if rows.shape[0] != N:
        raise GaeHipError(f"{who}: feat has {rows.shape[0]} rows, the CSR {N}")
    L = len(weights)
    keep, widths, prev = [graph_ptr, indptr, indices, rows], [], f_in
    w_ptrs, b_ptrs, ldws = (ctypes.c_void_p * max(L, 1))(), (ctypes.c_void_p * max(L, 1))(), (ctypes.c_int64 * max(L, 1))()
    for l, (W, b) in enumerate(zip(weights, biases)):
        W = _gpu(W, f"weights[{l}]").detach()
        if W.dtype != torch.float32 or W.dim() != 2 or W.shape[1] != prev or W.device != dev:
            raise GaeHipError(f"{who}: weights[{l}] must be fp32 [out, {prev}] on {dev}, got "
                              f"{W.dtype} {tuple(W.shape)} on {W.device}")
        if W.stride(1) != 1 or (W.shape[0] > 1 and W.stride(0) < W.shape[1]):
            W = W.contiguous()
        if b is not None:
            b = _gpu(b, f"biases[{l}]").detach()
            if b.dtype != torch.float32 or b.shape != (W.shape[0],) or b.device != dev:
                raise GaeHipError(f"{who}: biases[{l}] must be fp32 [{W.shape[0]}] on {dev}")
            b = b.contiguous()
        keep += [W, b]
        w_ptrs[l], b_ptrs[l] = W.data_ptr(), (b.data_ptr() if b is not None else None)
        ldws[l] = W.stride(0) if W.shape[0] > 1 else max(W.shape[1], 1)
        prev = int(W.shape[0])
        widths.append(prev)
    if graph_ids is not None:
        graph_ids = _gpu(graph_ids, "graph_ids")
        if graph_ids.dtype != torch.int64 or graph_ids.dim() != 1 or graph_ids.device != dev:
            raise GaeHipError(f"{who}: graph_ids must be an int64 [B] tensor on the set's device")
        graph_ids = graph_ids.contiguous()
        keep.append(graph_ids)
    B = G if graph_ids is None else graph_ids.numel()
    if max_graph_nodes is None:
        max_graph_nodes = int((graph_ptr[1:] - graph_ptr[:-1]).max()) if G > 0 else 0
    c_widths = (ctypes.c_int64 * max(L, 1))(*widths)
    c_acts = (ctypes.c_int * max(L, 1))(*acts)
    args = (_ptr(graph_ptr), G, N, indices.numel(), int(max_graph_nodes), _ptr(indptr), _ptr(indices), _ptr(rows), code,
            int(ldf), int(f_in), L, c_widths, w_ptrs, ldws, b_ptrs, c_acts, _NORMS[norm], _ptr(graph_ids), B)
    return args, keep, dev, B, widths, N, code, f_in


def embed_graphs_bwd_usable(f_in, widths, max_graph_nodes=0):
    """does gae_embed_graphs_bwd (K21) take the encoder ``f_in -> widths[0] -> ...``?  Narrower than
    ``embed_graphs_usable``: every layer's aggregated input and the weights in both orientations must fit the LDS, the
    weight-gradient tiles the registers.  Asks the library; no launch, no GPU."""
    widths = [int(w) for w in widths]
    arr = (ctypes.c_int64 * max(len(widths), 1))(*widths)
    return bool(_lib.load().gae_embed_graphs_bwd_usable(int(f_in), len(widths), arr, int(max_graph_nodes)))


def _launch_forward(head, dev, B, widths, N, code, norm):
    d = widths[-1] if widths else 0
    out = torch.empty(B, 3 * d, dtype=torch.float32, device=dev)
    args = head + (_ptr(out), max(3 * d, 1))
    embed_graphs.last_request = {"n_out": B, "widths": widths, "norm": norm, "dtype": code}
    with _on_device(dev):
        def launch():
            _lib.call("gae_embed_graphs", *args, _stream())
        if _ops.profiler is not None:
            _ops.profiler.wrap(("embed_graphs", N, B, tuple(widths)), launch)
        else:
            launch()
    return out


def embed_graphs_bwd(graph_ptr, indptr, indices, feat, weights, biases, acts, d_out, norm="none", graph_ids=None,
                     max_graph_nodes=None, want_weights=None, want_biases=None):
    """``(dWs, dbs)``: the gradients of the encoder's weights and biases for ``d_out`` [B, 3 d], the gradient of a loss
    with respect to the rows ``embed_graphs`` returns for the same arguments (K21, gae_embed_graphs_bwd: the encoder is
    recomputed per molecule in LDS, only the gradients reach memory).  ``want_weights`` / ``want_biases``: one flag per
    layer (None: all; a layer without bias never gets one); an entry that is not wanted comes back as None.  Same call,
    same bits.  Raises GaeHipError for shapes the kernel does not take (``embed_graphs_bwd_usable``)."""
    head, keep, dev, B, widths, N, code, f_in = _request("embed_graphs_bwd", graph_ptr, indptr, indices, feat, weights,
                                                          biases, acts, norm, graph_ids, max_graph_nodes)
    L = len(widths)
    if L == 0:
        raise GaeHipError("embed_graphs_bwd: an encoder of at least one layer expected")
    d = widths[-1]
    g = _gpu(d_out, "d_out").detach()
    if g.dtype != torch.float32 or tuple(g.shape) != (B, 3 * d) or g.device != dev:
        raise GaeHipError(f"embed_graphs_bwd: d_out must be fp32 [{B}, {3 * d}] on {dev}, got {g.dtype} "
                          f"{tuple(g.shape)} on {g.device}")
    if g.stride(1) != 1 or (B > 1 and g.stride(0) < 3 * d):
        g = g.contiguous()
    ldd = g.stride(0) if B > 1 else max(3 * d, 1)
    biases = [None] * L if biases is None else list(biases)
    want_weights = [True] * L if want_weights is None else [bool(w) for w in want_weights]
    want_biases = [True] * L if want_biases is None else [bool(w) for w in want_biases]
    ins = [f_in] + widths[:-1]
    dWs = [torch.empty(widths[l], ins[l], dtype=torch.float32, device=dev) if want_weights[l] else None for l in range(L)]
    dbs = [torch.empty(widths[l], dtype=torch.float32, device=dev) if want_biases[l] and biases[l] is not None else None
           for l in range(L)]
    c_widths = (ctypes.c_int64 * L)(*widths)
    nbytes = _ws_bytes("gae_embed_graphs_bwd_workspace_bytes", int(f_in), L, c_widths, B)
    ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
    p_dw, p_db, lddw = (ctypes.c_void_p * L)(), (ctypes.c_void_p * L)(), (ctypes.c_int64 * L)()
    for l in range(L):
        p_dw[l] = dWs[l].data_ptr() if dWs[l] is not None else None
        p_db[l] = dbs[l].data_ptr() if dbs[l] is not None else None
        lddw[l] = max(ins[l], 1)
    args = head + (_ptr(g), int(ldd), p_dw, lddw, p_db, _ptr(ws), ws.numel())
    embed_graphs_bwd.last_request = {"n_out": B, "widths": widths, "norm": norm, "dtype": code,
                                     "want_weights": want_weights, "want_biases": want_biases}
    with _on_device(dev):
        def launch():
            _lib.call("gae_embed_graphs_bwd", *args, _stream())
        if _ops.profiler is not None:
            _ops.profiler.wrap(("embed_graphs_bwd", N, B, tuple(widths)), launch)
        else:
            launch()
    del keep
    return dWs, dbs


embed_graphs_bwd.last_request = None


class _EmbedGraphs(torch.autograd.Function):
    """ops.embed_graphs with a backward: one gae_embed_graphs launch forward, one gae_embed_graphs_bwd call backward; the
    node holds the call's inputs and nothing per node"""

    @staticmethod
    def forward(ctx, static, L, *params):
        graph_ptr, indptr, indices, feat, acts, norm, graph_ids, max_graph_nodes = static
        weights, biases = list(params[:L]), list(params[L:])
        head, keep, dev, B, widths, N, code, _ = _request("embed_graphs", graph_ptr, indptr, indices, feat, weights,
                                                          biases, acts, norm, graph_ids, max_graph_nodes)
        out = _launch_forward(head, dev, B, widths, N, code, norm)
        ctx.static, ctx.L = static[:7] + (head[4],), L           # (max_graph_nodes as resolved by the forward)
        ctx.save_for_backward(*[p for p in params if p is not None])
        ctx.has_bias = [b is not None for b in biases]
        return out

    @staticmethod
    def backward(ctx, d_out):
        graph_ptr, indptr, indices, feat, acts, norm, graph_ids, max_graph_nodes = ctx.static
        L, saved = ctx.L, list(ctx.saved_tensors)
        weights = saved[:L]
        it = iter(saved[L:])
        biases = [next(it) if has else None for has in ctx.has_bias]
        need = ctx.needs_input_grad[2:]
        dWs, dbs = embed_graphs_bwd(graph_ptr, indptr, indices, feat, weights, biases, acts, d_out.float(), norm=norm,
                                    graph_ids=graph_ids, max_graph_nodes=max_graph_nodes,
                                    want_weights=need[:L], want_biases=need[L:])
        return (None, None) + tuple(dWs) + tuple(dbs)


def embed_graphs(graph_ptr, indptr, indices, feat, weights, biases, acts, norm="none", graph_ids=None,
                 max_graph_nodes=None):
    """[B, 3 d] fp32: row k = [mean | sum | max] over the nodes of member graph ``graph_ids[k]`` (None: every graph in
    order) of the embedding the encoder ``weights`` / ``biases`` / ``acts`` (per layer: [out, in] fp32, [out] or None,
    ACT_IDENTITY / ACT_RELU) gives on that graph alone.  ``graph_ptr`` int64 [G + 1], ``indptr`` / ``indices`` the int32
    CSR of the whole set (rows = destination, global column ids), ``feat`` uint8 or fp32 [N, F]: the arrays of a
    ``DeviceGraphDataset`` as they are.  ``norm``: "none" or "both" (D^-1/2 A D^-1/2 from the row lengths).
    ``max_graph_nodes``: host-side bound of the selected graphs' node counts (None: computed from ``graph_ptr``, one
    device read-back).  One launch; a graph's row has the same bits whatever else is embedded with it.
    With grad mode on and a weight or bias that requires a gradient the result carries one: its backward is one
    ``embed_graphs_bwd`` call (K21) that gives gradients to exactly the parameters that require them; the forward launch
    and its values are the same.  No gradient reaches ``feat``.
    Raises GaeHipError for CPU tensors and for shapes the kernel does not take (``embed_graphs_usable``; with a
    gradient also ``embed_graphs_bwd_usable``: never a detached result instead); there is no other route behind this
    function."""
    weights = list(weights)
    biases = [None] * len(weights) if biases is None else list(biases)
    if torch.is_grad_enabled() and any(isinstance(p, torch.Tensor) and p.requires_grad for p in weights + biases):
        if len(weights) != len(biases):
            raise GaeHipError("embed_graphs: weights, biases and acts must list the same layers")
        f_in = int(feat.shape[1]) if isinstance(feat, torch.Tensor) and feat.dim() == 2 else 0
        widths = [int(W.shape[0]) for W in weights]
        if not embed_graphs_bwd_usable(f_in, widths, 0):
            raise GaeHipError(f"embed_graphs: a gradient is asked for, but the backward kernel (gae_embed_graphs_bwd) "
                              f"does not take the encoder {f_in} -> {widths} (embed_graphs_bwd_usable); run under "
                              f"no_grad or use the chunked route")
        static = (graph_ptr, indptr, indices, feat, tuple(int(a) for a in acts), norm, graph_ids, max_graph_nodes)
        return _EmbedGraphs.apply(static, len(weights), *weights, *biases)
    head, keep, dev, B, widths, N, code, _ = _request("embed_graphs", graph_ptr, indptr, indices, feat, weights, biases,
                                                      acts, norm, graph_ids, max_graph_nodes)
    out = _launch_forward(head, dev, B, widths, N, code, norm)
    del keep
    return out


embed_graphs.last_request = None     # what the last call asked the library for (tests: which graphs took the kernel)
