"""What ops.decoder_topk (K16) and ops.decoder_rank (K18) share: the arguments that say who is a candidate -- the
embedding, the member windows, the CSR whose rows are left out -- and the size query / workspace / launch of their
entry points.  ``who`` names the caller in the messages.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import ctypes

import torch

import gae_dgl_amd.ops as _ops
from .. import _lib
from .._lib import GaeHipError
from ._base import _f32, _gpu, _on_device, _ptr, _rowmajor, _stream, _workspace


def _scope(Z, g, filter_graph, scope, exclude_edges, who):
    """(node_ptr, max_graph_nodes, csr) of the public functions: the member windows of the batched ``g`` for scope
    "graph", the CSR of ``filter_graph`` when its rows are left out"""
    if scope not in ("batch", "graph"):
        raise ValueError(f"scope: 'batch' or 'graph', not {scope!r}")
    _gpu(Z, "Z")
    if scope == "graph" and g is None:
        raise ValueError("scope='graph' needs the batched graph g")
    for name, gr in (("graph", g), ("filter_graph", filter_graph)):
        if gr is not None and gr.number_of_nodes() != Z.shape[0]:
            raise GaeHipError(f"{who}: Z has {Z.shape[0]} rows, the {name} {gr.number_of_nodes()} nodes")
    node_ptr, bound = (g.graph_ptr(), g.max_graph_nodes()) if scope == "graph" else (None, 0)
    csr = filter_graph.csr() if (exclude_edges and filter_graph is not None) else None
    return node_ptr, bound, csr


def _front(Z, node_ptr, max_graph_nodes, csr, exclude_self, who):
    """the checked common arguments of the raw functions: (Z, ldz, n, d, node_ptr, G, max_graph_nodes, indptr,
    indices, flags)"""
    Z = _f32(_gpu(Z, "Z"), f"{who}: Z")
    if Z.dim() != 2:
        raise GaeHipError(f"{who}: Z must be 2-D, got {tuple(Z.shape)}")
    Z, ldz = _rowmajor(Z, "Z")
    n, d = Z.shape
    if node_ptr is not None:
        node_ptr = _gpu(node_ptr, "node_ptr")
        if node_ptr.dtype != torch.int64 or node_ptr.dim() != 1 or node_ptr.numel() < 1:
            raise GaeHipError(f"{who}: node_ptr must be an int64 [G + 1] tensor")
        node_ptr = node_ptr.contiguous()
    G = node_ptr.numel() - 1 if node_ptr is not None else 0
    flags = _lib.TOPK_EXCLUDE_SELF if exclude_self else 0
    indptr = indices = None
    if csr is not None:
        indptr, indices = csr
        if indices.numel() == 0:
            indices = indptr             # no edge: a valid pointer that no row ever reads (the C ABI requires one)
        flags |= _lib.TOPK_EXCLUDE_EDGES
    return Z, max(ldz, d, 1), n, d, node_ptr, G, int(max_graph_nodes), indptr, indices, flags


def _run(symbol, args, key, dev):
    """size query -> workspace -> launch of the entry point ``symbol`` with ``args`` (all but workspace,
    workspace_bytes and stream), under the profiler as ``key`` when one is set"""
    with _on_device(dev):
        nbytes = ctypes.c_int64(0)
        _lib.check(getattr(_lib.load(), symbol)(*args, None, ctypes.byref(nbytes), None), f"{symbol} (size query)")
        ws = _workspace(int(nbytes.value), dev)

        def launch():
            _lib.call(symbol, *args, _ptr(ws), ctypes.byref(ctypes.c_int64(ws.numel())), _stream())
        if _ops.profiler is not None:
            _ops.profiler.wrap(key, launch)
        else:
            launch()
