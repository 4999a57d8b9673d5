"""Exact t-SNE of an embedding into the plane, on the device (K29, gae_tsne_*): neighbour lists from ``ops.knn``, their
conditional probabilities by an fp64 bisection per row, a symmetric sparse ``P``, and gradient iterations whose repulsive
term is an all-pairs sweep that stores nothing per pair -- no n x n matrix, no float atomics, one host read per group of
iterations.  ``GAE.map_nodes``, ``GAE.map_graphs``; ``metrics.neighbourhood_preservation`` scores a map.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import collections
import math

import torch

import gae_dgl_amd.ops as _ops
from .. import _lib
from .._lib import GaeHipError
from ._base import _f32, _gpu, _on_device, _ptr, _stream, _timed, _ws_bytes
from ._heads import _rows
from .knn import KNN_MAX_D, KNN_MAX_K

__all__ = ['TSNEResult', 'tsne', 'tsne_affinities', 'tsne_symmetrise', 'tsne_init', 'tsne_chunk', 'TSNEState']

TSNEResult = collections.namedtuple("TSNEResult", ["embedding", "kl_divergence", "kl_curve", "grad_norm", "n_iter",
                                                   "perplexities"])
TSNEResult.__doc__ = """embedding fp32 [n, 2]; kl_divergence: KL(P || Q) of the iterate the last update started from;
kl_curve: [(iteration, KL)] at every read of the status block; grad_norm: |g| of that update; n_iter: updates that
ran; perplexities fp64 [n]: what every row's bisection reached"""


def tsne_chunk(n):
    """gae_tsne_chunk(n): the column chunk width of the repulsion sweep, a function of n alone"""
    return _ws_bytes("gae_tsne_chunk", int(n))


def tsne_init(n, seed=0, device="cuda"):
    """fp32 [n, 2]: the start of gae_tsne_init, (2 u - 1) 1e-4 with u from the Philox stream keyed by (seed, element)"""
    dev = torch.device(device)
    Y = torch.empty(int(n), 2, dtype=torch.float32, device=dev)
    if n:
        with _on_device(dev):
            _lib.call("gae_tsne_init", _ptr(Y), 2, int(n), int(seed) & (2 ** 64 - 1), _stream())
    return Y


def tsne_affinities(index, dist2, perplexity):
    """(p fp32 [n, k], perplexities fp64 [n]): the conditional probabilities p_{j|i} of the neighbour lists ``index``
    int32 [n, k] / ``dist2`` fp32 [n, k] (``ops.knn``'s output under "l2"; -1 = padding), every row's entropy brought to
    log(``perplexity``) by an fp64 bisection on the device, and the perplexity each row reached.  1 <= k <= 64,
    1 <= perplexity < k."""
    index, dist2 = _gpu(index, "tsne_affinities: index"), _f32(_gpu(dist2, "tsne_affinities: dist2"), "tsne_affinities: dist2")
    if index.dtype != torch.int32 or index.dim() != 2 or index.shape != dist2.shape or index.device != dist2.device:
        raise GaeHipError(f"tsne_affinities: index int32 [n, k] and dist2 fp32 [n, k] on one device, got "
                          f"{index.dtype} {tuple(index.shape)} / {tuple(dist2.shape)}")
    index, dist2 = index.contiguous(), dist2.detach().contiguous()
    n, k = index.shape
    dev = index.device
    p = torch.empty(n, max(k, 1), dtype=torch.float32, device=dev)
    perp = torch.empty(n, dtype=torch.float64, device=dev)
    with _on_device(dev):
        def launch():
            _lib.call("gae_tsne_affinities", _ptr(index), _ptr(dist2), max(k, 1), n, k, float(perplexity), _ptr(p),
                      max(k, 1), _ptr(perp), _stream())
        _timed(("tsne_affinities", n, k), launch)
    return p[:, :k], perp


def tsne_symmetrise(index, p):
    """(indptr int32 [n + 1], indices int32 [nnz], values fp32 [nnz]): P = (P_{j|i} + P_{i|j}) / 2n as a CSR with sorted,
    merged rows.  Both directions are concatenated and stable-sorted by (row, col); a pair that both directions hold is
    two adjacent entries, added in fp64 -- no scatter-add, no float atomics.  Entries with p = 0 are dropped."""
    n, k = index.shape
    dev = index.device
    rows = torch.arange(n, device=dev, dtype=torch.int64).unsqueeze(1).expand(n, k)
    keep = (index >= 0) & (p > 0)
    r, c, v = rows[keep], index[keep].long(), p[keep].double()
    key = torch.cat([r * n + c, c * n + r])
    val = torch.cat([v, v])
    key, order = torch.sort(key, stable=True)
    val = val[order]
    if key.numel():
        first = torch.ones_like(key, dtype=torch.bool)
        first[1:] = key[1:] != key[:-1]
        twin = torch.zeros_like(val)
        twin[:-1] = torch.where(first[1:], torch.zeros_like(val[1:]), val[1:])    # a pair appears at most twice
        val = (val + twin)[first]
        key = key[first]
    val = (val / (2.0 * n)).float()
    r = torch.div(key, n, rounding_mode="floor")
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(r, minlength=n), 0)
    return indptr.int(), (key - r * n).int(), val


class TSNEState:
    """what the iterations of one fit keep on the device: Y (a strided view is updated in place), velocity, gains, the
    status block and the workspace.  ``step`` enqueues one iteration's three launches; ``read`` is the host read."""

    def __init__(self, Y, indptr, indices, values):
        self.Y = Y
        self.n = Y.shape[0]
        self.ldy = Y.stride(0) if self.n > 1 else 2
        self.indptr, self.indices, self.values = indptr, indices, values
        self.nnz = int(values.numel())
        dev = Y.device
        self.velocity = torch.zeros(self.n, 2, dtype=torch.float32, device=dev)
        self.gains = torch.ones(self.n, 2, dtype=torch.float32, device=dev)
        self.status = torch.zeros(_lib.TSNE_STATUS_WORDS, dtype=torch.int64, device=dev)
        self.ws = torch.empty(_ws_bytes("gae_tsne_workspace_bytes", self.n, self.nnz), dtype=torch.uint8, device=dev)
        self.chunk = tsne_chunk(self.n)
        self.chunks = -(-self.n // self.chunk)

    def repulsion(self, chunk_lo=0, chunk_hi=None, gated=True):
        _lib.call("gae_tsne_repulsion", _ptr(self.Y), self.ldy, self.n, int(chunk_lo),
                  self.chunks if chunk_hi is None else int(chunk_hi), _ptr(self.status) if gated else None, _ptr(self.ws),
                  self.ws.numel(), _stream())

    def partials(self):
        """fp32 [chunks, 3, n]: (fx, fy, z) per chunk and row, a view of the workspace's first region"""
        return self.ws[:12 * self.n * self.chunks].view(torch.float32).view(self.chunks, 3, self.n)

    def update(self, exaggeration, momentum, learning_rate, min_grad_norm=0.0):
        _lib.call("gae_tsne_update", _ptr(self.Y), self.ldy, self.n, _ptr(self.indptr), _ptr(self.indices),
                  _ptr(self.values), self.nnz, _ptr(self.velocity), _ptr(self.gains), float(exaggeration), float(momentum),
                  float(learning_rate), float(min_grad_norm), _ptr(self.status), _ptr(self.ws), self.ws.numel(), _stream())

    def step(self, exaggeration, momentum, learning_rate, min_grad_norm=0.0):
        self.repulsion()
        self.update(exaggeration, momentum, learning_rate, min_grad_norm)

    def read(self):
        """dict of the status block (one device-to-host copy)"""
        host = self.status.cpu()
        f = host.view(torch.float64)
        return {"done": int(host[0]), "iteration": int(host[1]), "nonfinite": int(host[2]), "p_log_d": float(f[4]),
                "log_z": float(f[5]), "grad2": float(f[6]), "z": float(f[7])}


def _check_y(Y, n, dev, who):
    Y = _f32(_gpu(Y, f"{who}: init"), f"{who}: init").detach()
    if Y.dim() != 2 or tuple(Y.shape) != (n, 2) or Y.device != dev:
        raise GaeHipError(f"{who}: init must be a [{n}, 2] tensor on {dev}, got {tuple(Y.shape)} on {Y.device}")
    return Y


def _pca_start(X, n, d, dev):
    """fp32 [n, 2]: sklearn's ``init="pca"`` -- the first two scores of ``ops.pca`` (K31) times the fp32 rounding of
    1e-4 / sigma, sigma = sqrt(lambda_1 (n - 1) / n) the standard deviation of the first score (from its variance, in
    fp64: no further pass); one fp32 product per entry.  d = 1: the second coordinate is zero.  n < 2: zeros"""
    Y = torch.zeros(n, 2, dtype=torch.float32, device=dev)
    if n < 2:
        return Y
    res = _ops.pca(X, min(2, d))
    lam = float(res.explained_variance[0])
    if not lam > 0.0:
        raise GaeHipError(f"tsne: init='pca' on a feature without variance (lambda_1 = {lam})")
    scale = torch.tensor(1e-4 / math.sqrt(lam * (n - 1) / n), dtype=torch.float64, device=dev).float()
    Z = res.transform(X)
    Y[:, :Z.shape[1]] = Z * scale
    return Y


def tsne(X, *, perplexity=20.0, n_iter=1000, learning_rate="auto", early_exaggeration=12.0, exaggeration_iters=250, seed=0,
         init=None, neighbours=None, metric="l2", min_grad_norm=1e-7, check_every=50):
    """``TSNEResult`` of exact t-SNE on the rows of ``X`` [n, d] (fp32, on the GPU; read in place when its inner stride is
    1): a map fp32 [n, 2].  Definitions and parameters are sklearn's: gains with +0.2 / x0.8 and a floor of 0.01,
    momentum 0.5 and exaggeration ``early_exaggeration`` for the first ``exaggeration_iters`` iterations, 0.8 and 1
    after; ``learning_rate="auto"`` is max(n / early_exaggeration / 4, 50); no recentring.  The repulsive term is the
    exact all-pairs sum (no Barnes-Hut tree).

    The affinities come from the ``k = min(n - 1, 64, ceil(3 perplexity))`` nearest neighbours (``ops.knn`` under
    ``metric`` = "l2", or a ``KNNResult`` of squared distances given as ``neighbours``).  ``ops.knn`` holds at most 64
    neighbours, which is why the default perplexity is 20: sklearn's default of 30 would ask for 90 and runs here on the
    64 nearest.  ``perplexity`` must be at least 1 and below k.

    ``init=None`` starts from (2 u - 1) 1e-4 with u from the library's Philox stream keyed by (``seed``, element);
    ``init=`` takes a [n, 2] tensor (copied); ``init="pca"`` starts from the first two principal scores (``ops.pca``, d <=
    128) divided by the standard deviation of the first and multiplied by 1e-4, sklearn's rule.  The iterations are enqueued in groups of ``check_every`` and the
    device's status block is read once per group (``kl_curve`` holds one point per read); the run stops early, on the
    device, once |g| <= ``min_grad_norm``.  The embedding has the same bits run to run, for any row stride of ``X``, any
    stream and any ``check_every``.  Two output dimensions only; 1 <= d <= 256.  ``n = 0`` gives an empty result,
    ``n = 1`` the start.  A non-finite row of ``X`` or a non-finite map raises GaeHipError; there is no CPU fallback."""
    for name, v in (("n_iter", n_iter), ("exaggeration_iters", exaggeration_iters)):
        if isinstance(v, bool) or int(v) != v or v < 0:
            raise ValueError(f"{name}: a non-negative integer, not {v!r}")
    if isinstance(check_every, bool) or int(check_every) != check_every or check_every < 1:
        raise ValueError(f"check_every: a positive integer, not {check_every!r}")
    if not float(perplexity) >= 1.0:
        raise ValueError(f"perplexity: at least 1, not {perplexity!r}")
    if not float(early_exaggeration) > 0.0:
        raise ValueError(f"early_exaggeration: positive, not {early_exaggeration!r}")
    if not float(min_grad_norm) >= 0.0:
        raise ValueError(f"min_grad_norm: non-negative, not {min_grad_norm!r}")
    if learning_rate != "auto" and not float(learning_rate) > 0.0:
        raise ValueError(f"learning_rate: 'auto' or a positive number, not {learning_rate!r}")
    if metric != "l2":
        raise ValueError(f"metric: 'l2' (squared Euclidean distances, as sklearn's default), not {metric!r}")
    with torch.no_grad():
        X, _, n, d = _rows(X, "tsne")
        dev = X.device
        if not 1 <= d <= KNN_MAX_D:
            raise GaeHipError(f"tsne: d = {d} outside 1..{KNN_MAX_D}")
        if n and not bool(torch.isfinite(X).all()):
            raise GaeHipError("tsne: X holds non-finite values")
        with _on_device(dev):
            if init is None:
                Y = tsne_init(n, seed, dev)
            elif isinstance(init, str):
                if init != "pca":
                    raise ValueError(f"init: None, 'pca' or a [n, 2] tensor, not {init!r}")
                Y = _pca_start(X, n, d, dev)
            else:
                Y = _check_y(init, n, dev, "tsne").clone().contiguous()
            empty = torch.empty(0, dtype=torch.float64, device=dev)
            if n < 2:
                return TSNEResult(Y, 0.0, [], 0.0, 0, empty if n == 0 else torch.ones(1, dtype=torch.float64, device=dev))
            k = min(n - 1, KNN_MAX_K, int(math.ceil(3.0 * float(perplexity))))
            if neighbours is None:
                nb = _ops.knn(X, k=k, metric="l2")
            else:
                nb = neighbours
                if nb.index.shape[0] != n or nb.index.shape[1] < 1:
                    raise GaeHipError(f"tsne: neighbours hold {tuple(nb.index.shape)} entries for n = {n} rows")
            p, perps = _ops.tsne_affinities(nb.index, nb.value, perplexity)
            indptr, indices, values = _ops.tsne_symmetrise(nb.index, p)
            v64 = values.double()
            sum_p = float(v64.sum())
            p_log_p = float((v64 * torch.log(v64)).sum())
            eta = max(n / float(early_exaggeration) / 4.0, 50.0) if learning_rate == "auto" else float(learning_rate)
            state = TSNEState(Y, indptr, indices, values)
            curve, last, enqueued = [], None, 0
            n_iter, check_every, exaggeration_iters = int(n_iter), int(check_every), int(exaggeration_iters)
            while enqueued < n_iter:
                group = min(check_every, n_iter - enqueued)
                for it in range(enqueued, enqueued + group):
                    early = it < exaggeration_iters

                    def launch():
                        state.step(float(early_exaggeration) if early else 1.0, 0.5 if early else 0.8, eta, min_grad_norm)
                    _timed(("tsne_step", n, state.nnz), launch)
                enqueued += group
                last = state.read()                                     # the one host read of the group
                if last["nonfinite"]:
                    raise GaeHipError(f"tsne: the map left the finite range ({last['nonfinite']} row updates) by iteration "
                                      f"{last['iteration']}")
                curve.append((last["iteration"], p_log_p + sum_p * last["log_z"] + last["p_log_d"]))
                if last["done"]:
                    break
    if last is None:
        return TSNEResult(Y, float("nan"), [], float("nan"), 0, perps)
    return TSNEResult(Y, curve[-1][1], curve, math.sqrt(last["grad2"]), last["iteration"], perps)
