"""Node clustering on the device (K23, gae_kmeans_*): k-means over the rows of an embedding -- k-means++ seeding,
Lloyd iterations and the assignment of new rows -- without the n x k distance matrix, without float atomics and with one
host read per group of iterations.  ``GAE.cluster_nodes``; ``metrics.clustering_metrics`` scores the labels (NMI, ARI,
accuracy).

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import collections

import torch

from .. import _lib
from .._lib import GaeHipError
from ._base import _f32, _gpu, _on_device, _ptr, _stream, _timed, _ws_bytes
from ._heads import _rows

__all__ = ['KMeansResult', 'kmeans_assign', 'kmeans', 'kmeans_init_pp']

KMeansResult = collections.namedtuple("KMeansResult", ["labels", "centers", "counts", "inertia", "n_iter", "converged",
                                                       "n_empty"])
KMeansResult.__doc__ = """labels int32 [n], centers fp32 [k, d], counts int64 [k] (rows per label), inertia (the
labels against the centres they were chosen with), n_iter, converged, n_empty (clusters without rows in the last
iteration; they kept their centre)"""

STATUS_WORDS = 6          # gae_kmeans_status: int64 done, iterations, changed, empty; double inertia, shift2


def _centres(C, d, dev, who):
    C = _f32(_gpu(C, f"{who}: centres"), f"{who}: centres")
    if C.dim() != 2 or C.shape[1] != d or C.device != dev:
        raise GaeHipError(f"{who}: centres must be a [k, {d}] tensor on {dev}, got {tuple(C.shape)} on {C.device}")
    return C


def _ws(n, d, k, dev):
    """a workspace of this call's own (the seeding and the steps of one run share it)"""
    nbytes = _ws_bytes("gae_kmeans_workspace_bytes", n, d, k)
    return torch.empty(int(nbytes), dtype=torch.uint8, device=dev)


def kmeans_assign(X, C):
    """(labels int32 [n], dist2 fp32 [n]): the nearest row of ``C`` [k, d] for every row of ``X`` [n, d] -- ties to the
    lower centre index -- and the squared distance to it, taken directly (no cancellation).  1 <= d <= 64, 1 <= k <= 256,
    k <= n; there is no CPU fallback."""
    with torch.no_grad():
        X, ldx, n, d = _rows(X, "kmeans_assign")
        C = _centres(C, d, X.device, "kmeans_assign").detach().contiguous()
        k = C.shape[0]
        dev = X.device
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        dist2 = torch.empty(n, dtype=torch.float32, device=dev)
        with _on_device(dev):
            ws = _ws(n, d, k, dev)

            def launch():
                _lib.call("gae_kmeans_assign", _ptr(X), ldx, n, d, _ptr(C), k, _ptr(labels), _ptr(dist2), _ptr(ws),
                          ws.numel(), _stream())
            _timed(("kmeans_assign", n, d, k), launch)
    return labels, dist2


def kmeans_init_pp(X, k, seed=0):
    """(centres fp32 [k, d], chosen int32 [k]): k-means++ seeding of gae_kmeans_init_pp -- the rows ``chosen`` of ``X``,
    a function of (X, k, seed) alone"""
    with torch.no_grad():
        X, ldx, n, d = _rows(X, "kmeans_init_pp")
        dev = X.device
        k = int(k)
        with _on_device(dev):
            ws = _ws(n, d, k, dev)
            return _init_pp(X, ldx, n, d, k, seed, ws)


def _init_pp(X, ldx, n, d, k, seed, ws):
    C = torch.empty(k, d, dtype=torch.float32, device=X.device)
    chosen = torch.empty(k, dtype=torch.int32, device=X.device)
    _lib.call("gae_kmeans_init_pp", _ptr(X), ldx, n, d, k, int(seed) & (2 ** 64 - 1), _ptr(C), _ptr(chosen), _ptr(ws),
              ws.numel(), _stream())
    return C, chosen


def _lloyd(X, ldx, n, d, C, tol_abs, max_iter, check_every, ws):
    """Lloyd iterations on ``C`` (in place) in groups of ``check_every`` launches; the status block is read once per
    group.  Returns (labels, status words)"""
    dev = X.device
    k = C.shape[0]
    labels = torch.full((n,), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(STATUS_WORDS, dtype=torch.int64, device=dev)
    enqueued = 0
    while True:
        group = min(check_every, max_iter - enqueued)
        for _ in range(group):
            _lib.call("gae_kmeans_step", _ptr(X), ldx, n, d, _ptr(C), k, _ptr(labels), _ptr(status), tol_abs, 0,
                      _ptr(ws), ws.numel(), _stream())
        enqueued += group
        host = status.cpu()                                    # the one host read of the group
        if int(host[0]) or enqueued >= max_iter:
            return labels, host


def kmeans(X, k, *, init="k-means++", n_init=1, max_iter=100, tol=1e-4, seed=0, check_every=8, check_finite=True):
    """KMeansResult of Lloyd's algorithm on the rows of ``X`` [n, d] (fp32, on the GPU; read in place when its inner
    stride is 1).  ``init``: "k-means++" (gae_kmeans_init_pp, seeded by ``seed``) or a [k, d] tensor of centres;
    ``n_init`` > 1 runs the seeds ``seed``, ``seed + 1``, ... and keeps the lowest inertia, the first among equals.
    An iteration stops the run when no label changed or when the centres moved by ``sum |c_new - c_old|^2 <= tol *
    mean_f Var_f(X)`` (sklearn's meaning of ``tol``; ``tol=0``: only when no label changed); at most ``max_iter``
    iterations.  The iterations are enqueued in groups of ``check_every`` and the device's status block is read once per
    group -- the result has the same bits for every group size, run to run and for any row stride of ``X``.
    A cluster that loses all its rows keeps its centre (``n_empty`` counts them).  1 <= d <= 64, 1 <= k <= 256, k <= n;
    non-finite input raises GaeHipError under ``check_finite``; there is no CPU fallback."""
    for name, v in (("n_init", n_init), ("max_iter", max_iter), ("check_every", check_every)):
        if isinstance(v, bool) or int(v) != v or v < 1:
            raise ValueError(f"{name}: a positive integer, not {v!r}")
    if not float(tol) >= 0.0:
        raise ValueError(f"tol: a non-negative number, not {tol!r}")
    with torch.no_grad():
        X, ldx, n, d = _rows(X, "kmeans")
        dev = X.device
        given = None
        if isinstance(init, torch.Tensor):
            given = _centres(init, d, dev, "kmeans").detach()
            if given.shape[0] != int(k):
                raise GaeHipError(f"kmeans: init holds {given.shape[0]} centres, k = {k}")
            n_init = 1
        elif init != "k-means++":
            raise ValueError(f"init: 'k-means++' or a [k, d] tensor, not {init!r}")
        k = int(k)
        if check_finite and not bool(torch.isfinite(X).all()):
            raise GaeHipError("kmeans: X holds non-finite values")
        # sklearn's tol: relative to the mean variance of the features; tol = 0 -> stop on unchanged labels only
        tol_abs = float(tol) * float(X.var(dim=0, unbiased=False).mean()) if float(tol) > 0 and n > 0 else -1.0
        best = None
        with _on_device(dev):
            ws = _ws(n, d, k, dev)
            for run in range(int(n_init)):
                C = given.clone().contiguous() if given is not None else _init_pp(X, ldx, n, d, k, int(seed) + run, ws)[0]
                labels, host = _lloyd(X, ldx, n, d, C, tol_abs, int(max_iter), int(check_every), ws)
                inertia = float(host[4:5].view(torch.float64))
                if best is None or inertia < best[2]:
                    best = (labels, C, inertia, host)
        labels, C, inertia, host = best
        counts = torch.bincount(labels.long(), minlength=k)
    return KMeansResult(labels, C, counts, inertia, int(host[1]), bool(int(host[0])), int(host[3]))
