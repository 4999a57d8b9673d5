"""How well a molecule set is reconstructed, per graph, in one launch (K20, gae_score_graphs): K19's encoder on every
selected member graph's own rows, then the inner-product decoder on the graph's own ordered pairs, ranked and scored in
LDS -- the counts behind ROC-AUC, the average precision and the no-dropout reconstruction loss of every graph.
``GAE.score_graphs`` / ``VGAE.score_graphs`` are the model-level entries, ``metrics.graph_score_summary`` the summary.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import collections
import ctypes

import torch

import gae_dgl_amd.ops as _ops
from .. import _lib
from ._base import _on_device, _ptr, _stream
from .embed import _request

__all__ = ['GraphScores', 'score_graphs_usable', 'score_graphs']

# device tensors of length B: loss fp32, auc / ap fp64, the four counts int64
GraphScores = collections.namedtuple("GraphScores", "loss auc ap n_pos n_neg wins ties")


def score_graphs_usable(f_in, widths, max_graph_nodes=0):
    """does gae_score_graphs take an encoder ``f_in -> widths[0] -> ...`` on graphs of at most ``max_graph_nodes`` nodes?
    As ``embed_graphs_usable``, and also ``widths = []``: the feature rows of width ``f_in`` <= 64 are the embedding.
    Asks the library; no launch, no GPU."""
    widths = [int(w) for w in widths]
    arr = (ctypes.c_int64 * max(len(widths), 1))(*widths)
    return bool(_lib.load().gae_score_graphs_usable(int(f_in), len(widths), arr, int(max_graph_nodes)))


def score_graphs(graph_ptr, indptr, indices, feat, weights=(), biases=None, acts=(), norm="none", graph_ids=None,
                 max_graph_nodes=None, exclude_self=True):
    """GraphScores of member graph ``graph_ids[k]`` (None: every graph in order), one entry per k.  Arguments as
    ``embed_graphs``; no layers (``weights = ()``) means ``feat`` (fp32 [N, d], d <= 64) IS the embedding Z.  On the
    graph's own ordered pairs (i != j when ``exclude_self``), a pair being a positive iff it is an entry of the graph's
    CSR: ``n_pos`` / ``n_neg``, ``wins`` / ``ties`` = the (positive, negative) pairs with the positive's logit above /
    exactly at the negative's, ``auc`` = (wins + ties / 2) / (n_pos n_neg), ``ap`` = the average precision with ties
    grouped, ``loss`` = the per-graph weighted BCE of ``decoder_bce_graphs`` without dropout.  NaN where a class is
    missing (loss: no positive); counts -1 and NaN for a graph the kernel refuses (above ``max_graph_nodes`` rows, a
    non-finite logit).  One launch; a graph's entries have the same bits whatever else is scored with it.
    Raises GaeHipError for CPU tensors and for shapes the kernel does not take (``score_graphs_usable``)."""
    head, keep, dev, B, widths, N, code, f_in = _request("score_graphs", graph_ptr, indptr, indices, feat, weights,
                                                         biases, acts, norm, graph_ids, max_graph_nodes)
    counts = torch.empty(B, 4, dtype=torch.int64, device=dev)
    ap = torch.empty(B, dtype=torch.float64, device=dev)
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    args = head + (1 if exclude_self else 0, _ptr(counts), _ptr(ap), _ptr(loss))
    score_graphs.last_request = {"n_out": B, "widths": widths, "norm": norm, "dtype": code, "f_in": f_in}
    with _on_device(dev):
        def launch():
            _lib.call("gae_score_graphs", *args, _stream())
        if _ops.profiler is not None:
            _ops.profiler.wrap(("score_graphs", N, B, tuple(widths)), launch)
        else:
            launch()
    del keep
    n_pos, n_neg, wins, ties = counts.unbind(1)
    both = (n_pos > 0) & (n_neg > 0)
    auc = (wins.double() + ties.double() / 2) / (n_pos * n_neg).clamp(min=1).double()
    auc = torch.where(both, auc, torch.full_like(auc, float("nan")))
    return GraphScores(loss, auc, ap, n_pos, n_neg, wins, ties)


score_graphs.last_request = None     # what the last call asked the library for (tests: which graphs took the kernel)
