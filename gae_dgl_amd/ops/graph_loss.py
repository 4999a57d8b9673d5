"""Per-member reconstruction loss of a batched graph (K15, gae_decoder_bce_graphs): the reference's loss of
train_inductive.py:44-48 taken on every member graph alone -- its own pairs, its own pos_weight, its own mean -- and
averaged over the members.  ``GAE.reconstruction_loss(g, scope="graph")``.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import torch

import gae_dgl_amd.ops as _ops
from .. import _lib
from .._lib import GaeHipError
from ._base import _f32, _gpu, _on_device, _ptr, _stream, _workspace, _ws_bytes

__all__ = ['decoder_bce_graphs_raw', 'DecoderBCEGraphsFunction', 'decoder_bce_graphs']

_SYNC = {}      # device -> int32[8] zeroed counters of gae_decoder_bce_graphs (every launch leaves them zero)


def _sync(device):
    """the launch counters of ``device``: zeroed once, outside any capture (a captured graph keeps the pointer)"""
    s = _SYNC.get(device)
    if s is None:
        if torch.cuda.is_current_stream_capturing():
            raise GaeHipError("decoder_bce_graphs: the first call on a device must run outside a HIP-graph capture "
                              "(warm-up step)")
        s = _SYNC[device] = torch.zeros(8, dtype=torch.int32, device=device)
    return s


def decoder_bce_graphs_raw(Z, mask, node_ptr, max_graph_nodes, csr, csc, want_grad=True, dropout=None, counts=None,
                           graph_loss=False):
    """(loss[1], per-member losses [G] or None, dZ or None) of gae_decoder_bce_graphs.
    ``node_ptr``: int64 [G + 1] member offsets on the device; ``max_graph_nodes``: host-side bound of the member sizes.
    ``dropout`` = (p, seed, offset, draw_counter): the mask is drawn inside the launch into ``mask`` ([n, d] output).
    ``counts``: true {nodes, ...} of a fixed-capacity batch (device int64)."""
    Z = _f32(_gpu(Z, "Z"), "decoder_bce_graphs: Z").contiguous()
    n, d = Z.shape
    if d > _ops.FUSED_MAX_D:
        raise GaeHipError(f"decoder_bce_graphs: embedding width {d} > {_ops.FUSED_MAX_D}")
    if mask is not None:
        mask = _f32(_gpu(mask, "mask"), "decoder_bce_graphs: mask")
        if mask.shape != Z.shape or not mask.is_contiguous():
            raise GaeHipError("decoder_bce_graphs: mask must be a contiguous [n, d] tensor")
    p_drop, seed, offset, draws = dropout if dropout is not None else (0.0, 0, 0, None)
    if p_drop and mask is None:
        raise GaeHipError("decoder_bce_graphs: in-launch dropout needs an [n, d] mask output buffer")
    node_ptr = _gpu(node_ptr, "node_ptr")
    if node_ptr.dtype != torch.int64 or node_ptr.dim() != 1 or node_ptr.numel() < 1:
        raise GaeHipError("decoder_bce_graphs: node_ptr must be an int64 [G + 1] tensor")
    node_ptr = node_ptr.contiguous()
    G = node_ptr.numel() - 1
    dev = Z.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    gl = torch.empty(G, dtype=torch.float32, device=dev) if graph_loss else None
    dZ = torch.empty(n, d, dtype=torch.float32, device=dev) if want_grad else None
    indptr, indices = csr
    t_indptr, t_indices = csc
    with _on_device(dev):
        nbytes = _ws_bytes("gae_decoder_bce_graphs_workspace_bytes", n, G, int(max_graph_nodes), d)
        ws = _workspace(nbytes, dev)
        sync = _sync(dev)

        def launch():
            _lib.call("gae_decoder_bce_graphs", _ptr(Z), _ptr(mask), max(d, 1), n, d, _ptr(node_ptr), G,
                      int(max_graph_nodes), _ptr(indptr), _ptr(indices), _ptr(t_indptr), _ptr(t_indices), _ptr(counts),
                      float(p_drop), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), _ptr(draws), _ptr(loss),
                      _ptr(gl), _ptr(dZ), max(d, 1), _ptr(ws), ws.numel(), _ptr(sync), _stream())
        if _ops.profiler is not None:
            _ops.profiler.wrap(("decoder_bce_graphs", n, d, want_grad), launch)
        else:
            launch()
    return loss, gl, dZ


class DecoderBCEGraphsFunction(torch.autograd.Function):
    """train_inductive.py:44-48 per member graph, averaged over the members (gae_decoder_bce_graphs): the gradient
    w.r.t. Z comes out of the same launch as the loss and is scaled in backward.  Second output: the per-member
    losses (NaN for members left out), not differentiable."""

    @staticmethod
    def forward(ctx, Z, mask, graph, dropout=None, counts=None, graph_loss=False):
        need = ctx.needs_input_grad[0]
        loss, gl, dZ = _ops.decoder_bce_graphs_raw(Z, mask, graph.graph_ptr(), graph.max_graph_nodes(), graph.csr(),
                                                   graph.csc(), want_grad=need, dropout=dropout, counts=counts,
                                                   graph_loss=graph_loss)
        ctx.save_for_backward(dZ)
        if gl is None:
            gl = loss.new_empty(0)
        ctx.mark_non_differentiable(gl)
        return loss.reshape(()), gl

    @staticmethod
    def backward(ctx, g, _g_graph):
        (dZ,) = ctx.saved_tensors
        if _ops._is_unit(g):
            return dZ, None, None, None, None, None
        return dZ * g, None, None, None, None, None


def decoder_bce_graphs(Z, mask, graph, dropout=None, counts=None, graph_loss=False):
    """mean over the member graphs of ``graph`` (``graph.graph_ptr()``; an unbatched graph is its own only member) of
    the weighted BCE of each member's own pairs.  ``dropout`` = (p, seed, offset, draw_counter): the mask is drawn
    inside the launch into ``mask``.  ``counts``: the true sizes of a fixed-capacity batch (default: the graph's
    ``batch_counts``).  ``graph_loss=True`` returns (loss, per-member losses [G])."""
    if counts is None:
        counts = getattr(graph, "batch_counts", None)
    loss, gl = _ops.DecoderBCEGraphsFunction.apply(Z, mask, graph, dropout, counts, bool(graph_loss))
    return (loss, gl) if graph_loss else loss
