"""Filtered link ranking without the N x N matrix (K18, gae_decoder_rank): for each query pair (i, j) how many
candidates c of node i -- decoder_topk's candidate rule, the target j left out -- have a logit z_i . z_c above, and how
many exactly at, the pair's own logit.  ``GAE.rank_links``; ``metrics.rank_metrics`` turns the counts into MRR, Hits@K,
mean rank and the exact all-negatives AUC.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import collections
import ctypes

import numpy as np
import torch

import gae_dgl_amd.ops as _ops
from .. import _lib
from .._lib import GaeHipError
from ._base import _f32, _gpu, _on_device, _ptr, _rowmajor, _stream, _workspace

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
    Z = _f32(_gpu(Z, "Z"), "decoder_rank: Z")
    if Z.dim() != 2:
        raise GaeHipError(f"decoder_rank: Z must be 2-D, got {tuple(Z.shape)}")
    Z, ldz = _rowmajor(Z, "Z")
    n, d = Z.shape
    dev = Z.device
    src, dst = _gpu(src, "src"), _gpu(dst, "dst")
    if src.dtype != torch.int64 or dst.dtype != torch.int64 or src.dim() != 1 or src.shape != dst.shape:
        raise GaeHipError("decoder_rank: src and dst must be int64 [m] tensors of one length")
    src, dst = src.contiguous(), dst.contiguous()
    m = src.numel()
    if node_ptr is not None:
        node_ptr = _gpu(node_ptr, "node_ptr")
        if node_ptr.dtype != torch.int64 or node_ptr.dim() != 1 or node_ptr.numel() < 1:
            raise GaeHipError("decoder_rank: node_ptr must be an int64 [G + 1] tensor")
        node_ptr = node_ptr.contiguous()
    G = node_ptr.numel() - 1 if node_ptr is not None else 0
    flags = _lib.TOPK_EXCLUDE_SELF if exclude_self else 0
    indptr = indices = None
    if csr is not None:
        indptr, indices = csr
        if indices.numel() == 0:
            indices = indptr             # no edge: a valid pointer that no row ever reads (the C ABI requires one)
        flags |= _lib.TOPK_EXCLUDE_EDGES
    mm = max(m, 1)
    score = torch.empty(mm, dtype=torch.float32, device=dev)
    counts = torch.empty(3, mm, dtype=torch.int64, device=dev)
    with _on_device(dev):
        lib = _lib.load()
        nbytes = ctypes.c_int64(0)
        args = (_ptr(Z), max(ldz, d, 1), n, d, _ptr(src), _ptr(dst), m, _ptr(node_ptr), G, int(max_graph_nodes),
                _ptr(indptr), _ptr(indices), flags, _ptr(score), _ptr(counts[0]), _ptr(counts[1]), _ptr(counts[2]))
        _lib.check(lib.gae_decoder_rank(*args, None, ctypes.byref(nbytes), None), "gae_decoder_rank (size query)")
        ws = _workspace(int(nbytes.value), dev)

        def launch():
            _lib.call("gae_decoder_rank", *args, _ptr(ws), ctypes.byref(ctypes.c_int64(ws.numel())), _stream())
        if _ops.profiler is not None:
            _ops.profiler.wrap(("decoder_rank", n, d, m), launch)
        else:
            launch()
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
    if scope not in ("batch", "graph"):
        raise ValueError(f"scope: 'batch' or 'graph', not {scope!r}")
    _gpu(Z, "Z")
    if scope == "graph" and g is None:
        raise ValueError("scope='graph' needs the batched graph g")
    fg = filter_graph if filter_graph is not None else g
    for name, gr in (("graph", g), ("filter_graph", fg)):
        if gr is not None and gr.number_of_nodes() != Z.shape[0]:
            raise GaeHipError(f"decoder_rank: Z has {Z.shape[0]} rows, the {name} {gr.number_of_nodes()} nodes")
    src, dst = _pairs_on(pairs, Z.device)
    node_ptr, bound = (g.graph_ptr(), g.max_graph_nodes()) if scope == "graph" else (None, 0)
    csr = fg.csr() if (exclude_edges and fg is not None) else None
    with torch.no_grad():
        return _ops.decoder_rank_raw(Z.detach(), src, dst, node_ptr, bound, csr, exclude_self=exclude_self)
