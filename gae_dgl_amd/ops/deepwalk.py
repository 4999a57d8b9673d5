"""The DeepWalk baseline (K37 gae_random_walks, K38 gae_sgns_accumulate / gae_sgns_update): uniform random walks over a
graph and a skip-gram embedding trained on them with negative sampling -- the row between spectral clustering and the
auto-encoders in the GAE / VGAE tables.  DeepWalk-LIKE: the trainer is synchronous mini-batch Adagrad with negatives shared
per walk, not word2vec's asynchronous loop (whose result depends on the order of its threads).  Walks are integer work, the
gradients of a batch meet in int64 fixed-point accumulators (32 fraction bits), so every run gives the same bits and equals
the numpy restatement of the header comment bit for bit.  No n x n object is formed.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import collections

import numpy as np
import torch

import gae_dgl_amd.ops as _ops
from .. import _lib
from .._lib import GaeHipError
from ._base import _gpu, _on_device, _ptr, _stream, _timed

__all__ = ['DeepWalkResult', 'SGNS_NOISE_BITS', 'random_walks', 'sgns_noise_weights', 'sgns_noise_table', 'sgns_init',
           'sgns_train', 'deepwalk']

SGNS_NOISE_BITS = 20                   # the noise weights are rint(2^20 count^power)
_ERRORS = ((_lib.DEEPWALK_ERR_COLUMN, "a column outside [0, n)"), (_lib.DEEPWALK_ERR_INDPTR, "a row pointer outside [0, nnz]"),
           (_lib.DEEPWALK_ERR_START, "a start outside [0, n)"),
           (_lib.DEEPWALK_ERR_RANGE, "a gradient element of 2^20 or more, or a non-finite one"),
           (_lib.DEEPWALK_ERR_NODE, "a walk-table entry outside [-1, n)"),
           (_lib.DEEPWALK_ERR_ORDER, "a walk-order entry outside [0, n_walks)"),
           (_lib.DEEPWALK_ERR_NONFINITE, "a non-finite table value after an update"))

DeepWalkResult = collections.namedtuple("DeepWalkResult", ["embedding", "context", "walks", "counts", "n_batches", "info"])
DeepWalkResult.__doc__ = """embedding = W fp32 [n, dim], context = C fp32 [n, dim], walks int32 [n_walks, L], counts int64 [n]
(visits of every node in the walks), n_batches (update steps taken), info: a dict with 'n_walks', 'visited', 'epochs' and the
Adagrad sums 'hw', 'hc' fp32 [n, dim]."""


def _int_arg(who, name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise GaeHipError(f"{who}: {name} = {v!r} outside {lo}..{hi}")
    return int(v)


def _raise_status(who, status):
    bits = int(status.cpu()[0])                            # the one read of the call / of the epoch
    if bits:
        what = ", ".join(text for bit, text in _ERRORS if bits & bit)
        raise GaeHipError(f"{who}: the device reported error flags 0x{bits:x} ({what})")


def random_walks(graph, *, walks_per_node=10, walk_length=40, starts=None, seed=0):
    """int32 [m r, L] uniform first-order random walks over ``graph`` (a Graph on the GPU) as its CSR stores it: duplicate
    edges count with their multiplicity, self-loops are stepped.  ``graph.csr()`` lists for every node the SOURCES of its
    incoming edges, so on a directed graph a walk steps against the edge direction; list both directions for an undirected
    walk.  ``starts`` int [m] (device tensor; None: every node), r = ``walks_per_node``, L = ``walk_length`` (1..65536).  Walk
    ``rep * m + s`` starts at ``starts[s]``; a node without entries ends its walk, the remaining positions are -1."""
    who = "random_walks"
    r = _int_arg(who, "walks_per_node", walks_per_node, 1, 2 ** 31 - 1)
    L = _int_arg(who, "walk_length", walk_length, 1, _lib.DEEPWALK_MAX_LENGTH)
    seed = _int_arg(who, "seed", seed, 0, 2 ** 64 - 1)
    with torch.no_grad():
        indptr, indices = graph.csr()
        _gpu(indptr, f"{who}: graph")
        dev = indptr.device
        n = indptr.shape[0] - 1
        if starts is not None:
            starts = _gpu(starts, f"{who}: starts")
            if starts.dim() != 1 or starts.dtype not in (torch.int32, torch.int64) or starts.device != dev:
                raise GaeHipError(f"{who}: starts must be an int32 / int64 [m] tensor on the graph's device")
            if starts.numel() and (int(starts.min()) < -2 ** 31 or int(starts.max()) >= 2 ** 31):
                raise GaeHipError(f"{who}: a start does not fit int32")
            starts = starts.to(torch.int32).contiguous()
        m = n if starts is None else starts.numel()
        if m * r >= 2 ** 31:
            raise GaeHipError(f"{who}: {m} starts times {r} walks is 2^31 or more")
        with _on_device(dev):
            wide = indptr.to(torch.int64).contiguous()
            indices = indices.contiguous()
            walks = torch.empty(m * r, L, dtype=torch.int32, device=dev)
            status = torch.zeros(_lib.DEEPWALK_STATUS_WORDS, dtype=torch.int64, device=dev)

            def launch():
                _lib.call("gae_random_walks", _ptr(wide), _ptr(indices), n, indices.shape[0], _ptr(starts), m, r, L, seed,
                          _ptr(walks), _ptr(status), _stream())
            _timed(("random_walks", n, m * r, L), launch)
            _raise_status(who, status)
    return walks


def sgns_noise_weights(counts, power=0.75):
    """int64 [n] on the host: rint(2^20 count^power) where the count is positive, 0 elsewhere (numpy fp64; the reference
    makes the same calls)"""
    c = np.asarray(counts, np.int64).astype(np.float64)
    w = np.zeros(c.shape[0], np.int64)
    seen = c > 0
    w[seen] = np.rint(np.float64(2.0) ** SGNS_NOISE_BITS * np.power(c[seen], np.float64(power))).astype(np.int64)
    return w


def _counts(walks, n, who):
    walks = _gpu(walks, f"{who}: walks")
    if walks.dim() != 2 or walks.dtype != torch.int32:
        raise GaeHipError(f"{who}: walks must be an int32 [n_walks, L] tensor, got {walks.dtype} {tuple(walks.shape)}")
    flat = walks.reshape(-1)
    flat = flat[flat >= 0].long()
    if flat.numel() and int(flat.max()) >= n:
        raise GaeHipError(f"{who}: the walks hold a node outside [0, {n})")
    return torch.bincount(flat, minlength=n)


def _table_of(counts, power, who):
    if not isinstance(power, (int, float)) or isinstance(power, bool) or not 0.0 <= power <= 1.0:
        raise GaeHipError(f"{who}: power = {power!r} outside [0, 1]")
    cum = np.zeros(counts.shape[0] + 1, np.int64)
    np.cumsum(sgns_noise_weights(counts.cpu().numpy(), power), out=cum[1:])
    return torch.from_numpy(cum).to(counts.device)


def sgns_noise_table(walks, n, power=0.75):
    """int64 cum [n + 1] on the walks' device: cum[i + 1] = cum[i] + rint(2^20 count_i^power) over the device bincount of the
    entries >= 0 (count 0: weight 0, so a node no walk visits is never drawn).  ``power`` = 0 is uniform over the visited
    nodes, 1 the corpus unigram, 0.75 word2vec's."""
    who = "sgns_noise_table"
    n = _int_arg(who, "n", n, 1, 2 ** 31 - 1)
    with torch.no_grad(), _on_device(_gpu(walks, f"{who}: walks").device):
        return _table_of(_counts(walks, n, who), power, who)


def sgns_init(n, dim, *, seed=0, device=None):
    """fp32 [n, dim] on the device: the Philox uniform draw in (-0.5 / dim, 0.5 / dim) the embedding table starts from"""
    who = "sgns_init"
    n = _int_arg(who, "n", n, 1, 2 ** 31 - 1)
    dim = _int_arg(who, "dim", dim, 1, _lib.SGNS_MAX_DIM)
    seed = _int_arg(who, "seed", seed, 0, 2 ** 64 - 1)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise GaeHipError(f"{who}: expected an AMD GPU device (gae_dgl_amd has no CPU fallback), got {dev}")
    with _on_device(dev):
        W = torch.empty(n, dim, dtype=torch.float32, device=dev)
        _lib.call("gae_sgns_init", _ptr(W), n, dim, seed, float(np.float32(0.5 / dim)), _stream())
    return W


def sgns_train(walks, cum, W, C, HW, HC, *, window=5, negatives=5, shared_negatives=16, epochs=3, batch_walks=256, lr=0.05,
               eps=1e-8, seed=0, first_epoch=0):
    """Trains the tables IN PLACE on ``walks`` int32 [n_walks, L] (2 <= L <= 64, -1: no node) for the epochs ``first_epoch`` ..
    ``first_epoch + epochs - 1`` and returns the number of batches.  ``cum`` int64 [n + 1]: ``sgns_noise_table``.  W (input
    table), C (context table), HW, HC (their Adagrad sums): fp32 [n, dim] contiguous device tensors.  Every batch of
    ``batch_walks`` consecutive positions of the epoch's keyed walk order is two launches: the gradients of all its walks into
    int64 accumulators, then one Adagrad sweep.  The status is read once per epoch; a gradient outside the fixed-point frame,
    a non-finite table or a CPU tensor raises GaeHipError."""
    who = "sgns_train"
    for name, t in (("walks", walks), ("cum", cum), ("W", W), ("C", C), ("HW", HW), ("HC", HC)):
        _gpu(t, f"{who}: {name}")
    if walks.dim() != 2 or walks.dtype != torch.int32 or not walks.is_contiguous():
        raise GaeHipError(f"{who}: walks must be a contiguous int32 [n_walks, L] tensor, got {walks.dtype} {tuple(walks.shape)}")
    if W.dim() != 2:
        raise GaeHipError(f"{who}: W must be [n, dim], got {tuple(W.shape)}")
    n, d = W.shape
    dev = W.device
    for name, t in (("W", W), ("C", C), ("HW", HW), ("HC", HC)):
        if t.dtype != torch.float32 or tuple(t.shape) != (n, d) or not t.is_contiguous() or t.device != dev:
            raise GaeHipError(f"{who}: {name} must be a contiguous fp32 [{n}, {d}] tensor on {dev}")
    if cum.dtype != torch.int64 or tuple(cum.shape) != (n + 1,) or not cum.is_contiguous() or cum.device != dev \
            or walks.device != dev:
        raise GaeHipError(f"{who}: cum must be a contiguous int64 [{n + 1}] tensor and the walks must be on {dev}")
    n_walks, L = walks.shape
    epochs = _int_arg(who, "epochs", epochs, 0, 2 ** 31 - 1)
    first_epoch = _int_arg(who, "first_epoch", first_epoch, 0, 2 ** 31 - 1 - epochs)
    B = _int_arg(who, "batch_walks", batch_walks, 1, 2 ** 31 - 1)
    seed = _int_arg(who, "seed", seed, 0, 2 ** 64 - 1)
    window = _int_arg(who, "window", window, -2 ** 63, 2 ** 63 - 1)             # (the library states the limits)
    K = _int_arg(who, "negatives", negatives, -2 ** 63, 2 ** 63 - 1)
    M = _int_arg(who, "shared_negatives", shared_negatives, -2 ** 63, 2 ** 63 - 1)
    if n_walks < 1:
        raise GaeHipError(f"{who}: no walks")
    lr, eps = float(np.float32(lr)), float(np.float32(eps))
    n_batches = 0
    with torch.no_grad(), _on_device(dev):
        if not (bool(torch.isfinite(W).all()) and bool(torch.isfinite(C).all()) and bool(torch.isfinite(HW).all())
                and bool(torch.isfinite(HC).all())):
            raise GaeHipError(f"{who}: a table holds a non-finite value")
        if int(cum[-1]) <= 0 or int(cum[0]) != 0:
            raise GaeHipError(f"{who}: the noise table is empty (cum[0] must be 0 and cum[n] positive)")
        AW = torch.zeros(n, d, dtype=torch.int64, device=dev)
        AC = torch.zeros(n, d, dtype=torch.int64, device=dev)
        order = torch.empty(n_walks, dtype=torch.int32, device=dev)
        status = torch.zeros(_lib.DEEPWALK_STATUS_WORDS, dtype=torch.int64, device=dev)
        for epoch in range(first_epoch, first_epoch + epochs):
            def run_epoch():
                _lib.call("gae_sgns_walk_order", n_walks, seed, epoch, _ptr(order), _stream())
                for first in range(0, n_walks, B):
                    _lib.call("gae_sgns_accumulate", _ptr(walks), n_walks, L, _ptr(order), first, min(B, n_walks - first),
                              _ptr(cum), n, d, window, K, M, seed, epoch, _ptr(W), _ptr(C), _ptr(AW), _ptr(AC), _ptr(status),
                              _stream())
                    _lib.call("gae_sgns_update", _ptr(W), _ptr(C), _ptr(HW), _ptr(HC), _ptr(AW), _ptr(AC), n, d, lr, eps,
                              _ptr(status), _stream())
            _timed(("sgns_epoch", n, d, n_walks, L), run_epoch)
            n_batches += -(-n_walks // B)
            _raise_status(who, status)
    return n_batches


def deepwalk(graph, dim=64, *, walks_per_node=10, walk_length=40, window=5, negatives=5, shared_negatives=16, epochs=3,
             batch_walks=256, lr=0.05, eps=1e-8, noise_power=0.75, seed=0, walks=None):
    """``DeepWalkResult`` of ``graph`` (a Graph on the GPU): ``walks_per_node`` walks of ``walk_length`` (2..64) nodes from
    every node (``random_walks``; or the given ``walks`` int32 [n_walks, L]), the noise table of their visit counts to the
    ``noise_power`` and ``epochs`` of ``sgns_train`` on a ``dim``-wide (1..128) table.  W starts as a Philox uniform draw in
    (-0.5 / dim, 0.5 / dim), C and the Adagrad sums at zero; every positive pair (two valid positions at most ``window``
    apart) meets ``negatives`` noise nodes in expectation, through ``shared_negatives`` (16, 32, 48 or 64) draws per walk.
    Rows no walk visits keep their initial values.  The same arguments give the same bits."""
    who = "deepwalk"
    dim = _int_arg(who, "dim", dim, 1, _lib.SGNS_MAX_DIM)
    seed = _int_arg(who, "seed", seed, 0, 2 ** 64 - 1)
    with torch.no_grad():
        indptr = graph.csr()[0]
        _gpu(indptr, f"{who}: graph")
        dev = indptr.device
        n = indptr.shape[0] - 1
        if n < 1:
            raise GaeHipError(f"{who}: the graph has no nodes")
        if walks is None:
            L = _int_arg(who, "walk_length", walk_length, 2, _lib.SGNS_MAX_LENGTH)
            walks = _ops.random_walks(graph, walks_per_node=walks_per_node, walk_length=L, seed=seed)
        else:
            walks = _gpu(walks, f"{who}: walks")
            if walks.device != dev:
                raise GaeHipError(f"{who}: the walks are on {walks.device}, the graph on {dev}")
        with _on_device(dev):
            counts = _counts(walks, n, who)
            cum = _table_of(counts, noise_power, who)
            W = _ops.sgns_init(n, dim, seed=seed, device=dev)
            C, HW, HC = (torch.zeros(n, dim, dtype=torch.float32, device=dev) for _ in range(3))
            walks = walks.contiguous()
            n_batches = _ops.sgns_train(walks, cum, W, C, HW, HC, window=window, negatives=negatives,
                                        shared_negatives=shared_negatives, epochs=epochs, batch_walks=batch_walks, lr=lr, eps=eps,
                                        seed=seed)
            info = {"n_walks": walks.shape[0], "visited": int((counts > 0).sum()), "epochs": epochs, "hw": HW, "hc": HC}
    return DeepWalkResult(W, C, walks, counts, n_batches, info)
