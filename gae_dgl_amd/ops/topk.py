"""Top-k link prediction without the N x N matrix (K16, gae_decoder_topk): for every node the k candidates j with the
largest logit z_i . z_j of the decoder of gae.py:69-72, with the known edges, the node itself and (scope "graph") the
other members of a batch left out.  ``GAE.predict_links``.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import ctypes

import torch

import gae_dgl_amd.ops as _ops
from .. import _lib
from .._lib import GaeHipError
from ._base import _f32, _gpu, _on_device, _ptr, _rowmajor, _stream, _workspace

__all__ = ['decoder_topk_raw', 'decoder_topk']

MAX_K = 64


def decoder_topk_raw(Z, k, node_ptr=None, max_graph_nodes=0, csr=None, exclude_self=True):
    """(score fp32 [n, k], index int64 [n, k]) of gae_decoder_topk.  ``node_ptr``: int64 [G + 1] member offsets on the
    device (scope "graph") or None (scope "batch"); ``csr``: (indptr, indices) whose rows are left out, or None."""
    Z = _f32(_gpu(Z, "Z"), "decoder_topk: Z")
    if Z.dim() != 2:
        raise GaeHipError(f"decoder_topk: Z must be 2-D, got {tuple(Z.shape)}")
    Z, ldz = _rowmajor(Z, "Z")
    n, d = Z.shape
    k = int(k)
    dev = Z.device
    if node_ptr is not None:
        node_ptr = _gpu(node_ptr, "node_ptr")
        if node_ptr.dtype != torch.int64 or node_ptr.dim() != 1 or node_ptr.numel() < 1:
            raise GaeHipError("decoder_topk: node_ptr must be an int64 [G + 1] tensor")
        node_ptr = node_ptr.contiguous()
    G = node_ptr.numel() - 1 if node_ptr is not None else 0
    flags = _lib.TOPK_EXCLUDE_SELF if exclude_self else 0
    indptr = indices = None
    if csr is not None:
        indptr, indices = csr
        if indices.numel() == 0:
            indices = indptr             # no edge: a valid pointer that no row ever reads (the C ABI requires one)
        flags |= _lib.TOPK_EXCLUDE_EDGES
    kk = max(k, 1)
    score = torch.empty(n, kk, dtype=torch.float32, device=dev)
    index = torch.empty(n, kk, dtype=torch.int64, device=dev)
    with _on_device(dev):
        lib = _lib.load()
        nbytes = ctypes.c_int64(0)
        args = (_ptr(Z), max(ldz, d, 1), n, d, k, _ptr(node_ptr), G, int(max_graph_nodes), _ptr(indptr),
                _ptr(indices), flags, _ptr(score), _ptr(index), kk)
        _lib.check(lib.gae_decoder_topk(*args, None, ctypes.byref(nbytes), None), "gae_decoder_topk (size query)")
        ws = _workspace(int(nbytes.value), dev)

        def launch():
            _lib.call("gae_decoder_topk", *args, _ptr(ws), ctypes.byref(ctypes.c_int64(ws.numel())), _stream())
        if _ops.profiler is not None:
            _ops.profiler.wrap(("decoder_topk", n, d, k), launch)
        else:
            launch()
    return score, index


def decoder_topk(Z, k, g=None, *, scope="batch", exclude_self=True, exclude_edges=True):
    """(score [n, k], index [n, k]): for every row i of the embedding ``Z`` the k nodes j with the largest logit
    z_i . z_j (sigmoid(score) is the decoder's probability, gae.py:71), rows sorted by score descending and equal scores
    by ascending j; fewer than k candidates pad with index -1 / score -inf.
    ``scope="graph"``: candidates only inside i's own member graph of a batched ``g``.  ``exclude_self``: j != i.
    ``exclude_edges``: the in-edges of i in ``g`` (CSR row i) are left out; without a graph there is nothing to leave out.
    No N x N matrix is formed, and there is no CPU fallback."""
    if scope not in ("batch", "graph"):
        raise ValueError(f"scope: 'batch' or 'graph', not {scope!r}")
    if not 1 <= int(k) <= MAX_K:
        raise GaeHipError(f"decoder_topk: k = {k} outside 1..{MAX_K}")
    _gpu(Z, "Z")
    if scope == "graph" and g is None:
        raise ValueError("scope='graph' needs the batched graph g")
    if g is not None and g.number_of_nodes() != Z.shape[0]:
        raise GaeHipError(f"decoder_topk: Z has {Z.shape[0]} rows, the graph {g.number_of_nodes()} nodes")
    node_ptr, bound = (g.graph_ptr(), g.max_graph_nodes()) if scope == "graph" else (None, 0)
    csr = g.csr() if (exclude_edges and g is not None) else None
    with torch.no_grad():
        return _ops.decoder_topk_raw(Z.detach(), k, node_ptr, bound, csr, exclude_self=exclude_self)
