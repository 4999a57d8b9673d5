"""Top-k link prediction without the N x N matrix (K16, gae_decoder_topk): for every node the k candidates j with the
largest logit z_i . z_j of the decoder of gae.py:69-72, with the known edges, the node itself and (scope "graph") the
other members of a batch left out.  ``GAE.predict_links``.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import torch

import gae_dgl_amd.ops as _ops
from .._lib import GaeHipError
from ._base import _ptr
from ._candidates import _front, _run, _scope

__all__ = ['decoder_topk_raw', 'decoder_topk']

MAX_K = 64


def decoder_topk_raw(Z, k, node_ptr=None, max_graph_nodes=0, csr=None, exclude_self=True):
    """(score fp32 [n, k], index int64 [n, k]) of gae_decoder_topk.  ``node_ptr``: int64 [G + 1] member offsets on the
    device (scope "graph") or None (scope "batch"); ``csr``: (indptr, indices) whose rows are left out, or None."""
    Z, ldz, n, d, node_ptr, G, bound, indptr, indices, flags = _front(Z, node_ptr, max_graph_nodes, csr, exclude_self,
                                                                      "decoder_topk")
    k = int(k)
    kk = max(k, 1)
    score = torch.empty(n, kk, dtype=torch.float32, device=Z.device)
    index = torch.empty(n, kk, dtype=torch.int64, device=Z.device)
    _run("gae_decoder_topk", (_ptr(Z), ldz, n, d, k, _ptr(node_ptr), G, bound, _ptr(indptr), _ptr(indices), flags,
                              _ptr(score), _ptr(index), kk), ("decoder_topk", n, d, k), Z.device)
    return score, index


def decoder_topk(Z, k, g=None, *, scope="batch", exclude_self=True, exclude_edges=True):
    """(score [n, k], index [n, k]): for every row i of the embedding ``Z`` the k nodes j with the largest logit
    z_i . z_j (sigmoid(score) is the decoder's probability, gae.py:71), rows sorted by score descending and equal scores
    by ascending j; fewer than k candidates pad with index -1 / score -inf.
    ``scope="graph"``: candidates only inside i's own member graph of a batched ``g``.  ``exclude_self``: j != i.
    ``exclude_edges``: the in-edges of i in ``g`` (CSR row i) are left out; without a graph there is nothing to leave out.
    No N x N matrix is formed, and there is no CPU fallback."""
    if not 1 <= int(k) <= MAX_K:
        raise GaeHipError(f"decoder_topk: k = {k} outside 1..{MAX_K}")
    node_ptr, bound, csr = _scope(Z, g, g, scope, exclude_edges, "decoder_topk")
    with torch.no_grad():
        return _ops.decoder_topk_raw(Z.detach(), k, node_ptr, bound, csr, exclude_self=exclude_self)
