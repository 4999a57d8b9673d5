"""Filtered link ranking without the N x N matrix (K18, gae_decoder_rank): for each query pair (i, j) how many
candidates c of node i -- decoder_topk's candidate rule, the target j left out -- have a logit z_i . z_c above, and how
many exactly at, the pair's own logit.  ``GAE.rank_links``; ``metrics.rank_metrics`` turns the counts into MRR, Hits@K,
mean rank and the exact all-negatives AUC.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import collections

import numpy as np
import torch

import gae_dgl_amd.ops as _ops
from .._lib import GaeHipError
from ._base import _gpu, _ptr
from ._candidates import _front, _run, _scope

__all__ = ['RankResult', 'decoder_rank_raw', 'decoder_rank']

RankResult = collections.namedtuple("RankResult", ["score", "greater", "equal", "candidates"])


def _pairs_on(pairs, dev):
    """``pairs`` ([2, m]; tensor or array, any device, any integer type) as two contiguous int64 rows on ``dev``"""
    if not isinstance(pairs, torch.Tensor):
        pairs = torch.from_numpy(np.ascontiguousarray(np.asarray(pairs)))
    if pairs.dtype.is_floating_point or pairs.dtype == torch.bool or pairs.dtype.is_complex:
        raise GaeHipError(f"decoder_rank: pairs must hold integers, not {pairs.dtype}")
    if pairs.dim() != 2 or pairs.shape[0] != 2:
        raise GaeHipError(f"decoder_rank: pairs must be [2, m], got {tuple(pairs.shape)}")
    pairs = pairs.to(device=dev, dtype=torch.int64)
    return pairs[0].contiguous(), pairs[1].contiguous()


def decoder_rank_raw(Z, src, dst, node_ptr=None, max_graph_nodes=0, csr=None, exclude_self=True):
    """RankResult (score fp32 [m], greater / equal / candidates int64 [m]) of gae_decoder_rank for the queries
    (src[q], dst[q]): int64 [m] tensors on Z's device.  ``node_ptr``: int64 [G + 1] member offsets on the device (scope
    "graph") or None (scope "batch"); ``csr``: (indptr, indices) whose rows are left out, or None."""
    Z, ldz, n, d, node_ptr, G, bound, indptr, indices, flags = _front(Z, node_ptr, max_graph_nodes, csr, exclude_self,
                                                                      "decoder_rank")
    src, dst = _gpu(src, "src"), _gpu(dst, "dst")
    if src.dtype != torch.int64 or dst.dtype != torch.int64 or src.dim() != 1 or src.shape != dst.shape:
        raise GaeHipError("decoder_rank: src and dst must be int64 [m] tensors of one length")
    src, dst = src.contiguous(), dst.contiguous()
    m = src.numel()
    mm = max(m, 1)
    score = torch.empty(mm, dtype=torch.float32, device=Z.device)
    counts = torch.empty(3, mm, dtype=torch.int64, device=Z.device)
    _run("gae_decoder_rank", (_ptr(Z), ldz, n, d, _ptr(src), _ptr(dst), m, _ptr(node_ptr), G, bound, _ptr(indptr),
                              _ptr(indices), flags, _ptr(score), _ptr(counts[0]), _ptr(counts[1]), _ptr(counts[2])),
         ("decoder_rank", n, d, m), Z.device)
    return RankResult(score[:m], counts[0, :m], counts[1, :m], counts[2, :m])


def decoder_rank(Z, pairs, g=None, *, filter_graph=None, scope="batch", exclude_self=True, exclude_edges=True):
    """RankResult(score [m], greater [m], equal [m], candidates [m]) for the query pairs ``pairs`` ([2, m]: row 0 the
    sources i, row 1 the targets j; tensor or array on any device): ``score`` is the logit z_i . z_j, ``greater`` /
    ``equal`` count the candidates c of i, j itself left out, with z_i . z_c above / exactly at it, ``candidates`` is
    how many there are.  rank = 1 + greater + equal / 2 (``metrics.rank_metrics``).
    Candidates follow ``decoder_topk``: ``scope="graph"`` keeps them inside i's member graph of the batched ``g``,
    ``exclude_self`` drops c = i, ``exclude_edges`` drops the in-edges of i in ``filter_graph`` (default ``g``) --
    pass the FULL graph, held-out edges included, for the filtered protocol: the target is ranked even when it is one
    of the filtered edges.  An index outside [0, n) gives score NaN and counts -1.
    No m x n matrix is formed, and there is no CPU fallback."""
    fg = filter_graph if filter_graph is not None else g
    node_ptr, bound, csr = _scope(Z, g, fg, scope, exclude_edges, "decoder_rank")
    src, dst = _pairs_on(pairs, Z.device)
    with torch.no_grad():
        return _ops.decoder_rank_raw(Z.detach(), src, dst, node_ptr, bound, csr, exclude_self=exclude_self)
