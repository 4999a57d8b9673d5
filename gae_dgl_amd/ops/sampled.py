"""Unbiased sampled reconstruction loss (K17, gae_decoder_bce_sampled): the fused loss's edge term exactly, its
all-pairs term from m keyed-random partners per row, O((E + N m) d) per step instead of O(N^2 d).  Its expectation is
the loss of ``decoder_bce`` (same label, pos_weight, mean and dropout); at m = N it equals it up to rounding.
``GAE.reconstruction_loss(g, samples=m)``, ``VGAE.loss(g, samples=m)``, ``parallel.sharded_loss(..., samples=m)``.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import ctypes

import torch

import gae_dgl_amd.ops as _ops
from .. import _lib
from .._lib import GaeHipError
from ._base import _f32, _gpu, _on_device, _ptr, _stream, _workspace
from .loss import _is_unit

__all__ = ['decoder_bce_sampled_raw', 'DecoderBCESampledFunction', 'decoder_bce_sampled',
           'ShardedDecoderBCESampledFunction', 'sharded_decoder_bce_sampled']


def decoder_bce_sampled_raw(Z, mask, csr, csc, pos_weight, samples, seed=0, offset=0, draws=None, dropout_p=0.0,
                            want_grad=True, row_begin=0, n_local=None, partners=False):
    """(loss[1], dZ [n_local, d] or None, partners int32 [n_local, m] or None) of gae_decoder_bce_sampled.
    ``Z`` / ``mask``: the full [n, d] arrays; ``csr`` / ``csc``: (indptr, indices) of the rows [row_begin, row_begin +
    n_local) -- indptr of those rows (it may be a slice of a whole graph's, offsets into the same indices), global
    column ids.  ``dropout_p`` > 0: the mask of this draw is drawn in the launch into ``mask`` (an [n, d] buffer).
    ``draws``: the device draw counter (int64 [1]), advanced by one by the launch; the sampler's draw is
    offset + *draws."""
    Z = _f32(_gpu(Z, "Z"), "decoder_bce_sampled: Z").contiguous()
    if Z.dim() != 2:
        raise GaeHipError(f"decoder_bce_sampled: Z must be 2-D, got {tuple(Z.shape)}")
    n, d = Z.shape
    if mask is not None:
        mask = _f32(_gpu(mask, "mask"), "decoder_bce_sampled: mask").contiguous()
        if mask.shape != Z.shape:
            raise GaeHipError("decoder_bce_sampled: the mask must have Z's shape")
    if dropout_p and mask is None:
        raise GaeHipError("decoder_bce_sampled: in-kernel dropout needs an [n, d] mask output buffer")
    n_local = n - int(row_begin) if n_local is None else int(n_local)
    m = int(samples)
    dev = Z.device
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    dZ = torch.empty(n_local, d, dtype=torch.float32, device=dev) if want_grad else None
    part = torch.empty(n_local, m, dtype=torch.int32, device=dev) if partners else None
    indptr, indices = csr
    t_indptr, t_indices = csc if csc is not None else (None, None)
    args = (_ptr(Z), _ptr(mask), max(d, 1), n, d, int(row_begin), n_local, m, _ptr(indptr), _ptr(indices),
            _ptr(t_indptr), _ptr(t_indices), float(pos_weight), float(dropout_p), int(seed) & (2 ** 64 - 1),
            int(offset) & (2 ** 64 - 1), _ptr(draws), _ptr(loss), _ptr(dZ), max(d, 1), _ptr(part))
    with _on_device(dev):
        lib = _lib.load()
        nbytes = ctypes.c_int64(0)
        _lib.check(lib.gae_decoder_bce_sampled(*args, None, ctypes.byref(nbytes), None),
                   "gae_decoder_bce_sampled (size query)")
        if _ops.current_step().tails:
            _ops.current_step().flush_loss_tails()     # an earlier deferred loss may still read the cached workspace
        ws = _workspace(int(nbytes.value), dev)

        def launch():
            _lib.call("gae_decoder_bce_sampled", *args, _ptr(ws), ctypes.byref(ctypes.c_int64(ws.numel())), _stream())
        if _ops.profiler is not None:
            _ops.profiler.wrap(("decoder_bce_sampled", n, d, m, want_grad), launch)
        else:
            launch()
    return loss, dZ, part


def _check_samples(samples, n):
    m = int(samples)
    if not 1 <= m <= n:
        raise GaeHipError(f"decoder_bce_sampled: samples = {samples} outside 1..{n} (the number of nodes)")
    return m


def _row_csr(csr, row_range):
    """the CSR of the rows [r0, r0 + n_local): a view of indptr, the same indices (offsets stay absolute)"""
    if row_range is None or csr is None:
        return csr
    r0, nl = row_range
    ip, ix = csr
    return ip[r0:r0 + nl + 1], ix


class DecoderBCESampledFunction(torch.autograd.Function):
    """The sampled estimate of DecoderBCEFunction's loss: label from the graph's CSR, pos_weight, dropout as there; the
    gradient w.r.t. Z comes from the same launch and is scaled in backward."""

    @staticmethod
    def forward(ctx, Z, mask, graph, samples, dropout=None, row_range=None):
        if getattr(graph, "batch_counts", None) is not None:
            raise GaeHipError("decoder_bce_sampled: fixed-capacity batches are not supported")
        n = graph.number_of_nodes()
        nnz = graph.number_of_edges()
        if Z.shape[0] != n:
            raise GaeHipError(f"decoder_bce_sampled: Z has {Z.shape[0]} rows, the graph {n} nodes")
        m = _check_samples(samples, n)
        pw = (float(n) * float(n) - float(nnz)) / float(nnz)                 # train_inductive.py:46
        p_drop, seed, offset, draws = dropout if dropout is not None else (0.0, 0, 0, None)
        r0, nl = row_range if row_range is not None else (0, n)
        need = ctx.needs_input_grad[0]
        loss, dZ, _ = _ops.decoder_bce_sampled_raw(Z, mask, _row_csr(graph.csr(), row_range),
                                                   _row_csr(graph.csc(), row_range) if need else None, pw, m, seed,
                                                   offset, draws, p_drop, want_grad=need, row_begin=r0, n_local=nl)
        if need and row_range is not None and (r0, nl) != (0, n):
            full = torch.zeros(n, Z.shape[1], dtype=torch.float32, device=Z.device)
            full[r0:r0 + nl] = dZ
            dZ = full
        ctx.save_for_backward(dZ)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dZ,) = ctx.saved_tensors
        if _is_unit(g):
            return dZ, None, None, None, None, None
        return dZ * g, None, None, None, None, None


def decoder_bce_sampled(Z, mask, graph, samples, dropout=None, row_range=None):
    """Unbiased estimate of ``decoder_bce(Z, mask, graph)`` from ``samples`` = m partners per row (1 <= m <= N): the
    edge term exactly, the all-pairs term from m distinct keyed-random partners per row weighted N / m.
    ``dropout`` = (p, seed, offset, draw_counter): the sampler's draw is offset + *draw_counter and the counter advances
    by one per call (also with p = 0, then the mask is ``mask`` or none); p > 0 draws the dropout mask of that counter
    into ``mask`` (an [n, d] buffer), the stream of ``decoder_bce``.  None: no dropout, a fixed draw 0.
    ``row_range`` = (row_begin, n_local): this block's share of the loss; the gradient is nonzero on these rows only."""
    if Z.shape[1] > _ops.FUSED_MAX_D:
        raise GaeHipError(f"decoder_bce_sampled: embedding width {Z.shape[1]} > {_ops.FUSED_MAX_D}")
    return _ops.DecoderBCESampledFunction.apply(Z, mask, graph, samples, dropout, row_range)


class ShardedDecoderBCESampledFunction(torch.autograd.Function):
    """ShardedDecoderBCEFunction with the sampled estimate: Zt = Z (.) mask all-gathered, this rank's row block of the
    estimate (the rows form), the shares summed by a scalar all-reduce.  Every rank draws the same partners (same seed,
    same device counter), so its dZ rows have the bits of one GPU's."""

    @staticmethod
    def forward(ctx, z_local, mask_local, sg, n_edges_global, samples, seed, draws):
        p = sg.part
        zt_local = z_local if mask_local is None else z_local * mask_local
        full = sg.allgather_rows(zt_local)
        n = p.n
        m = _check_samples(samples, n)
        pw = (float(n) * float(n) - float(n_edges_global)) / float(n_edges_global)
        need = ctx.needs_input_grad[0]
        loss, dzt, _ = _ops.decoder_bce_sampled_raw(full[:n], None, sg.csr_global("fwd"),
                                                    sg.csr_global("bwd") if need else None, pw, m, seed, 0, draws,
                                                    want_grad=need, row_begin=p.r0, n_local=p.n_local)
        sg.allreduce_sum(loss)
        ctx.save_for_backward(dzt, mask_local)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        dzt, mask_local = ctx.saved_tensors
        dz = dzt if _is_unit(g) else dzt * g
        if mask_local is not None:
            dz = dz * mask_local
        return dz, None, None, None, None, None, None


def sharded_decoder_bce_sampled(z_local, mask_local, sg, samples, seed=0, n_edges_global=None):
    """the sampled loss on a row-sharded graph; the draw counter lives on ``sg`` (created on first use, advanced by
    every call)"""
    if n_edges_global is None:
        n_edges_global = sg.n_edges_global()
    draws = getattr(sg, "_loss_draws", None)
    if draws is None or draws.device != z_local.device:
        draws = sg._loss_draws = torch.zeros(1, dtype=torch.int64, device=z_local.device)
    return _ops.ShardedDecoderBCESampledFunction.apply(z_local, mask_local, sg, n_edges_global, samples, seed, draws)
