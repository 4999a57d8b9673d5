"""The molecule feature of a whole resident set in one launch (K19, gae_embed_graphs): for every selected member graph
the complete GCN encoder on that graph's own rows followed by the [mean | sum | max] readout -- the node embeddings
never reach memory.  ``GAE.embed_graphs`` is the model-level entry; ``python -m gae_dgl_amd.embed`` the script.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import ctypes

import torch

import gae_dgl_amd.ops as _ops
from .. import _lib
from .._lib import GaeHipError
from ._base import _gpu, _on_device, _ptr, _stream

__all__ = ['EMBED_MAX_LAYERS', 'EMBED_MAX_WIDTH', 'EMBED_MAX_NODES', 'embed_graphs_usable', 'embed_graphs']

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


def embed_graphs(graph_ptr, indptr, indices, feat, weights, biases, acts, norm="none", graph_ids=None,
                 max_graph_nodes=None):
    """[B, 3 d] fp32: row k = [mean | sum | max] over the nodes of member graph ``graph_ids[k]`` (None: every graph in
    order) of the embedding the encoder ``weights`` / ``biases`` / ``acts`` (per layer: [out, in] fp32, [out] or None,
    ACT_IDENTITY / ACT_RELU) gives on that graph alone.  ``graph_ptr`` int64 [G + 1], ``indptr`` / ``indices`` the int32
    CSR of the whole set (rows = destination, global column ids), ``feat`` uint8 or fp32 [N, F]: the arrays of a
    ``DeviceGraphDataset`` as they are.  ``norm``: "none" or "both" (D^-1/2 A D^-1/2 from the row lengths).
    ``max_graph_nodes``: host-side bound of the selected graphs' node counts (None: computed from ``graph_ptr``, one
    device read-back).  One launch; a graph's row has the same bits whatever else is embedded with it.
    Raises GaeHipError for CPU tensors and for shapes the kernel does not take (``embed_graphs_usable``); there is no
    other route behind this function."""
    head, keep, dev, B, widths, N, code, _ = _request("embed_graphs", graph_ptr, indptr, indices, feat, weights, biases,
                                                      acts, norm, graph_ids, max_graph_nodes)
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
    del keep
    return out


embed_graphs.last_request = None     # what the last call asked the library for (tests: which graphs took the kernel)
