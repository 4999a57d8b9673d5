"""The decoded graph without the N x N matrix (K22, gae_decoder_threshold_count / _fill): the reconstruction
A_hat = 1[sigmoid(z_i . z_j) >= p] of the decoder of gae.py:69-72 as a CSR -- for every node the candidates (decoder_topk's
candidate rule) whose logit is at or above a threshold, in ascending column order, with their logits.
``GAE.reconstruct``; ``metrics.reconstruction_metrics`` turns it into precision / recall / F1 and the fraction of member
graphs reproduced exactly.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import collections
import ctypes
import math

import torch

import gae_dgl_amd.ops as _ops
from .. import _lib
from .._lib import GaeHipError
from ._base import _on_device, _ptr, _stream
from ._candidates import _front, _scope

__all__ = ['DecodedLinks', 'decoder_threshold_raw', 'decoder_threshold', 'threshold_of_prob']


class DecodedLinks(collections.namedtuple("DecodedLinks", ["indptr", "index", "score"])):
    """CSR of the decoded graph: row i (a destination, as in the library's CSR) lists ``index[indptr[i]:indptr[i + 1]]``
    (int32, ascending) with the logits ``score`` (fp32); ``indptr`` is int64 [n + 1]"""
    __slots__ = ()

    def pairs(self):
        """(row int64 [nnz], col int64 [nnz]) of the listed pairs"""
        n = self.indptr.numel() - 1
        rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=self.indptr.device),
                                       self.indptr[1:] - self.indptr[:-1])
        return rows, self.index.long()


def threshold_of_prob(prob):
    """the logit at which sigmoid reaches ``prob`` in (0, 1): log(p / (1 - p)) in fp64, rounded to fp32 (0.5 -> 0.0)"""
    p = float(prob)
    if not 0.0 < p < 1.0:
        raise ValueError(f"prob: a probability inside (0, 1), not {prob!r}")
    return float(torch.tensor(math.log(p / (1.0 - p)), dtype=torch.float64).to(torch.float32))


def decoder_threshold_raw(Z, threshold, node_ptr=None, max_graph_nodes=0, csr=None, exclude_self=True, splits=0,
                          capacity=None, out=None, max_pairs=None):
    """(indptr int64 [n + 1], index int32 [capacity], score fp32 [capacity], total) of gae_decoder_threshold_count
    followed by gae_decoder_threshold_fill on one workspace.  ``node_ptr``: int64 [G + 1] member offsets on the device
    (scope "graph") or None; ``csr``: (indptr, indices) whose rows are left out, or None; ``splits``: 0 = auto or 1..16
    column splits.  ``capacity``: how many pairs the fill may write (default: all ``total`` of them; reading the total
    is one host sync); ``out``: (index, score) buffers of at least ``capacity`` entries to fill instead of new ones;
    ``max_pairs``: raise GaeHipError, before anything is allocated or filled, when the total exceeds it."""
    Z, ldz, n, d, node_ptr, G, bound, indptr, indices, flags = _front(Z, node_ptr, max_graph_nodes, csr, exclude_self,
                                                                      "decoder_threshold")
    dev = Z.device
    sel = (_ptr(Z), ldz, n, d, float(threshold), _ptr(node_ptr), G, bound, _ptr(indptr), _ptr(indices), flags,
           int(splits))
    row_ptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
    with _on_device(dev):
        nbytes = ctypes.c_int64(0)
        _lib.check(_lib.load().gae_decoder_threshold_count(*sel, None, None, ctypes.byref(nbytes), None),
                   "gae_decoder_threshold_count (size query)")
        # private to this call, not the shared scratch: it carries the offsets from the count to the fill
        ws = torch.empty(max(int(nbytes.value), 16), dtype=torch.uint8, device=dev)
        ws_bytes = ctypes.c_int64(ws.numel())

        def count():
            _lib.call("gae_decoder_threshold_count", *sel, _ptr(row_ptr), _ptr(ws), ctypes.byref(ws_bytes), _stream())
        if _ops.profiler is not None:
            _ops.profiler.wrap(("decoder_threshold_count", n, d), count)
        else:
            count()
        total = int(row_ptr[n])                                # the one host sync
        if max_pairs is not None and total > int(max_pairs):
            raise GaeHipError(f"decoder_threshold: {total} pairs at threshold {float(threshold):g}, more than max_pairs "
                              f"= {int(max_pairs)}: raise the threshold or max_pairs ({12 * total} bytes of output)")
        cap = total if capacity is None else int(capacity)
        if out is not None:
            index, score = out
        else:
            index = torch.empty(max(cap, 0), dtype=torch.int32, device=dev)
            score = torch.empty(max(cap, 0), dtype=torch.float32, device=dev)

        def fill():
            _lib.call("gae_decoder_threshold_fill", *sel, _ptr(row_ptr), _ptr(index), _ptr(score), cap, _ptr(ws),
                      ctypes.byref(ws_bytes), _stream())
        if _ops.profiler is not None:
            _ops.profiler.wrap(("decoder_threshold_fill", n, d), fill)
        else:
            fill()
    return row_ptr, index, score, total


def decoder_threshold(Z, threshold, g=None, *, scope="batch", exclude_self=True, exclude_edges=False, max_pairs=2 ** 27):
    """DecodedLinks(indptr int64 [n + 1], index int32 [nnz], score fp32 [nnz]): for every row i of the embedding ``Z``
    the nodes j with logit z_i . z_j >= ``threshold`` (sigmoid(score) is the decoder's probability, gae.py:71; a logit
    equal to the threshold is listed), columns ascending within a row; rows are destinations, as in the library's CSR.
    The listed logits have the bits ``decoder_topk`` gives those pairs.
    Candidates follow ``decoder_topk``: ``scope="graph"`` keeps them inside i's member graph of the batched ``g``,
    ``exclude_self`` drops j = i, ``exclude_edges`` drops the in-edges of i in ``g``; NaN and -inf logits are never
    listed.  ``max_pairs``: the call counts first and raises GaeHipError when more pairs than this would be listed (12
    bytes each; an untrained model decodes to a nearly complete graph).
    No N x N matrix is formed, the cost in memory is the output; there is no CPU fallback."""
    node_ptr, bound, csr = _scope(Z, g, g, scope, exclude_edges, "decoder_threshold")
    threshold = float(threshold)
    if math.isnan(threshold):
        raise GaeHipError("decoder_threshold: threshold is NaN")
    if isinstance(max_pairs, bool) or int(max_pairs) != max_pairs or max_pairs < 0:
        raise ValueError(f"max_pairs: a non-negative number of pairs, not {max_pairs!r}")
    with torch.no_grad():
        row_ptr, index, score, _ = _ops.decoder_threshold_raw(Z.detach(), threshold, node_ptr, bound, csr,
                                                              exclude_self=exclude_self, max_pairs=int(max_pairs))
    return DecodedLinks(row_ptr, index, score)
