"""Circular fingerprints of a resident molecule set (K33, gae_fingerprint_graphs): a Morgan / Weisfeiler-Lehman hash of
every atom's neighbourhoods up to ``radius`` bonds, folded into ``n_bits`` slots per molecule -- the ECFP family of
descriptor on what the set stores (featuriser rows as atom invariants, the block-diagonal CSR as neighbourhoods).  The
set holds no bond orders: these are NOT RDKit's ECFP bits.  ``DeviceGraphDataset.fingerprints`` is the set-level entry,
``ops.tanimoto_knn`` the search over the words, ``python -m gae_dgl_amd.fingerprint`` the script.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import torch

from .. import _lib
from .._lib import GaeHipError
from ._base import _gpu, _on_device, _ptr, _stream, _timed, _ws_bytes

__all__ = ['FINGERPRINT_MAX_RADIUS', 'FINGERPRINT_N_BITS', 'fingerprint_graphs', 'fingerprint_unpack',
           'fingerprint_fold']

FINGERPRINT_MAX_RADIUS = 8
FINGERPRINT_N_BITS = (64, 128, 256, 512, 1024, 2048)


def _check_options(radius, n_bits, who):
    if isinstance(radius, bool) or int(radius) != radius or not 0 <= radius <= FINGERPRINT_MAX_RADIUS:
        raise GaeHipError(f"{who}: radius must be an integer in 0..{FINGERPRINT_MAX_RADIUS}, not {radius!r}")
    if isinstance(n_bits, bool) or int(n_bits) != n_bits or int(n_bits) not in FINGERPRINT_N_BITS:
        raise GaeHipError(f"{who}: n_bits must be one of {FINGERPRINT_N_BITS}, not {n_bits!r}")


def fingerprint_graphs(graph_ptr, indptr, indices, feat, *, radius=2, n_bits=1024, counts=False, graph_ids=None):
    """int32 [B, n_bits / 32] bit words (bit j of word w is slot 32 w + j), or with ``counts=True`` int32 [B, n_bits]
    slot counts: row k is the circular fingerprint of member graph ``graph_ids[k]`` (None: every graph in order; any
    order, repeats allowed).  ``graph_ptr`` int64 [G + 1], ``indptr`` / ``indices`` the int32 CSR of the whole set,
    ``feat`` uint8 or fp32 [N, F], read in place when its inner stride is 1: the arrays of a ``DeviceGraphDataset`` as
    they are.  Atom ids at radius 0 hash the feature row (a uint8 feature as its fp32 value, so both storages agree);
    radius r mixes an atom's id with the commutative sum over its CSR row, so the result does not depend on the order of
    atoms or edges.  Integer arithmetic only: the same bits run to run.  radius 0..8, n_bits a power of two in 64..2048;
    there is no other route behind this function."""
    who = "fingerprint_graphs"
    _check_options(radius, n_bits, who)
    graph_ptr = _gpu(graph_ptr, "graph_ptr")
    dev = graph_ptr.device
    for name, t in (("indptr", indptr), ("indices", indices), ("feat", feat)):
        if _gpu(t, name).device != dev:
            raise GaeHipError(f"{who}: {name} is on {t.device}, graph_ptr on {dev}")
    if graph_ptr.dtype != torch.int64 or graph_ptr.dim() != 1 or graph_ptr.numel() < 1:
        raise GaeHipError(f"{who}: graph_ptr must be an int64 [G + 1] tensor")
    if indptr.dtype != torch.int32 or indices.dtype != torch.int32 or indptr.dim() != 1 or indices.dim() != 1 \
            or indptr.numel() < 1:
        raise GaeHipError(f"{who}: indptr / indices must be int32 vectors (the CSR of the resident set)")
    if feat.dim() != 2 or feat.dtype not in (torch.uint8, torch.float32) or feat.shape[1] < 1:
        raise GaeHipError(f"{who}: feat must be uint8 or fp32 [N, F >= 1], got {feat.dtype} {tuple(feat.shape)}")
    graph_ptr, indptr, indices = graph_ptr.contiguous(), indptr.contiguous(), indices.contiguous()
    feat = feat.detach()
    N, F = feat.shape
    if N != indptr.numel() - 1:
        raise GaeHipError(f"{who}: feat has {N} rows, the CSR {indptr.numel() - 1}")
    if feat.stride(1) != 1 or (N > 1 and feat.stride(0) < F):
        feat = feat.contiguous()
    ldf = feat.stride(0) if N > 1 else F
    if graph_ids is not None:
        graph_ids = _gpu(graph_ids, "graph_ids")
        if graph_ids.dtype != torch.int64 or graph_ids.dim() != 1 or graph_ids.device != dev:
            raise GaeHipError(f"{who}: graph_ids must be an int64 [B] tensor on the set's device")
        graph_ids = graph_ids.contiguous()
    G = graph_ptr.numel() - 1
    B = G if graph_ids is None else graph_ids.numel()
    width = int(n_bits) if counts else int(n_bits) // 32
    out = torch.empty(B, width, dtype=torch.int32, device=dev)
    code = _lib.U8 if feat.dtype == torch.uint8 else _lib.F32
    with _on_device(dev):
        ws = torch.empty(_ws_bytes("gae_fingerprint_workspace_bytes", N), dtype=torch.uint8, device=dev)

        def launch():
            _lib.call("gae_fingerprint_graphs", _ptr(graph_ptr), G, N, indices.numel(), _ptr(indptr), _ptr(indices),
                      _ptr(feat), code, int(ldf), int(F), _ptr(graph_ids), B, int(radius), int(n_bits), int(bool(counts)),
                      _ptr(out), width, _ptr(ws), ws.numel(), _stream())
        _timed(("fingerprint_graphs", N, B, int(radius), int(n_bits)), launch)
    return out


def fingerprint_unpack(words, dtype=torch.float32):
    """0 / 1 columns [B, 32 W] of ``dtype`` from int32 bit words [B, W] (torch glue, host or device tensors): column
    32 w + j is bit j of word w.  The heads take the fp32 result as it is."""
    if not isinstance(words, torch.Tensor) or words.dtype != torch.int32 or words.dim() != 2:
        raise GaeHipError("fingerprint_unpack: int32 bit words [B, W] expected")
    shifts = torch.arange(32, dtype=torch.int32, device=words.device)
    bits = (words.unsqueeze(-1) >> shifts) & 1
    return bits.reshape(words.shape[0], words.shape[1] * 32).to(dtype)


def fingerprint_fold(fp, n_bits, counts=None):
    """the fingerprint at a smaller power of two ``n_bits`` (torch glue, host or device tensors): ``fp`` int32 counts
    [B, N] are summed, int32 bit words [B, N / 32] are ORed.  Because a slot is ``id mod n_bits`` this equals the
    fingerprint computed at that width directly.  ``counts=None`` tells the two apart by ``fp.shape[1]`` (words have
    fewer than 64 columns, counts more); a [B, 64] input is either 64 counts or the words of 2048 bits and must say."""
    if not isinstance(fp, torch.Tensor) or fp.dtype != torch.int32 or fp.dim() != 2:
        raise GaeHipError("fingerprint_fold: an int32 [B, n_bits] count or [B, n_bits / 32] word tensor expected")
    if isinstance(n_bits, bool) or int(n_bits) != n_bits or int(n_bits) not in FINGERPRINT_N_BITS:
        raise GaeHipError(f"fingerprint_fold: n_bits must be one of {FINGERPRINT_N_BITS}, not {n_bits!r}")
    n_bits, width = int(n_bits), fp.shape[1]
    if counts is None:
        if width == 64:
            raise GaeHipError("fingerprint_fold: 64 columns are 64 counts or the words of 2048 bits: pass counts=")
        counts = width > 64
    as_words = not counts
    have = width * 32 if as_words else width
    if have not in FINGERPRINT_N_BITS or have < n_bits:
        raise GaeHipError(f"fingerprint_fold: a fingerprint of {have} slots cannot be folded to {n_bits}")
    if as_words:
        out = fp.reshape(fp.shape[0], have // n_bits, n_bits // 32)
        acc = out[:, 0].clone()
        for p in range(1, out.shape[1]):
            acc |= out[:, p]
        return acc
    return fp.reshape(fp.shape[0], have // n_bits, n_bits).sum(1, dtype=torch.int32)
