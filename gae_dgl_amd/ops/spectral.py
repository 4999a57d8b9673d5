"""Spectral embedding of a graph (K32, gae_spectral_*): the k algebraically largest eigenpairs of the symmetric
normalised adjacency S = D^-1/2 (A + sigma I) D^-1/2 by Chebyshev-filtered block subspace iteration with a Rayleigh-Ritz
step, in fp64 on the device -- the "spectral clustering" baseline of the GAE / VGAE tables.  Every launch is a stated
sequence of operations (the same bits run to run, no rocSOLVER / rocSPARSE call, no host linear algebra); the host reads
one 64-byte status block per checked iteration.  The smallest eigenpairs of the normalised Laplacian I - S are (1 - theta,
the same vectors).

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import collections

import torch

from .. import _lib
from .._lib import GaeHipError
from ._base import _on_device, _ptr, _stream, _timed, _ws_bytes

__all__ = ['SpectralResult', 'spectral_embedding', 'SPECTRAL_MAX_K', 'SPECTRAL_MAX_B', 'SPECTRAL_MAX_DEGREE']

SPECTRAL_MAX_K, SPECTRAL_MAX_B, SPECTRAL_MAX_DEGREE = _lib.SPECTRAL_MAX_K, _lib.SPECTRAL_MAX_B, _lib.SPECTRAL_MAX_DEGREE
STATUS_WORDS = _lib.SPECTRAL_STATUS_WORDS
_SCALINGS = {"none": _lib.SPECTRAL_SCALE_NONE, "degree": _lib.SPECTRAL_SCALE_DEGREE, "value": _lib.SPECTRAL_SCALE_VALUE}

SpectralResult = collections.namedtuple("SpectralResult", [
    "embedding", "vectors", "values", "residuals", "n_iter", "n_spmm", "converged", "info"])
SpectralResult.__doc__ = """embedding fp32 [n, k] (the vectors scaled per ``scaling``, rounded); vectors fp64 [n, k]
(orthonormal up to rounding; the entry of largest magnitude of each is positive); values fp64 [k] (the Ritz values,
descending); residuals fp64 [k] (||S v - theta v||_2); n_iter outer iterations; n_spmm block products with S; converged:
every residual <= tol; info 0."""


def _int_in(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise GaeHipError(f"spectral_embedding: {name} = {v!r} outside {lo}..{hi}")
    return v


def spectral_embedding(graph, k=16, *, self_loops=False, oversample=None, degree=8, tol=1e-8, max_iter=200, seed=0,
                       check_every=1, scaling="none", drop_first=False):
    """``SpectralResult`` of ``graph`` (a Graph on the GPU, symmetric: every edge listed in both directions; duplicate edges
    count with their multiplicity in A and in the degrees).  ``self_loops``: sigma = 1, the GCN operator.  The block is
    b = k + ``oversample`` columns wide (default max(8, k); b even, <= 128, <= n).  An outer iteration: one product AV = S V,
    the Gram pair, the b x b solve (fp64 Cholesky, K31's Jacobi), the rotation with its residuals, then -- unless the top k
    converged -- a Chebyshev filter of ``degree`` (<= 12) products on [-1, min(theta_b, theta_k - 0.02)].  The host reads the
    status after every ``check_every``-th iteration and stops at the first checked one whose top k residuals are all <= ``tol``
    (absolute: ||S|| <= 1), or at ``max_iter`` (then ``converged`` is False; nothing is raised).  ``scaling``: "none",
    "degree" (row i times (deg_i + sigma)^-1/2: the random-walk eigenvectors) or "value" (column c times sqrt(max(theta_c,
    0)): z_i . z_j is the rank-k approximation of S).  ``drop_first``: compute k + 1 pairs and drop the top one (k <= 63).
    An asymmetric graph, a limit outside its range, a factorisation that breaks down or a non-finite value raises
    GaeHipError; there is no CPU fallback."""
    who = "spectral_embedding"
    _int_in("k", k, 1, SPECTRAL_MAX_K - (1 if drop_first else 0))
    kk = k + (1 if drop_first else 0)
    if oversample is None:
        oversample = max(8, kk)
        oversample += (kk + oversample) & 1
        oversample = min(oversample, SPECTRAL_MAX_B - kk)
    _int_in("oversample", oversample, 0, SPECTRAL_MAX_B)
    b = kk + oversample
    if b & 1 or not 2 <= b <= SPECTRAL_MAX_B:
        raise GaeHipError(f"{who}: the block width k + oversample = {b} must be even and in 2..{SPECTRAL_MAX_B}")
    _int_in("degree", degree, 1, SPECTRAL_MAX_DEGREE)
    _int_in("max_iter", max_iter, 1, 1 << 30)
    _int_in("check_every", check_every, 1, 1 << 30)
    _int_in("seed", seed, 0, (1 << 64) - 1)
    if scaling not in _SCALINGS:
        raise GaeHipError(f"{who}: scaling = {scaling!r}, not one of 'none', 'degree', 'value'")
    tol = float(tol)
    if not 0.0 <= tol < float("inf"):
        raise GaeHipError(f"{who}: tol = {tol!r} must be finite and >= 0")
    sigma = 1.0 if self_loops else 0.0
    with torch.no_grad():
        indptr, indices = graph.csr()
        t_indptr, t_indices = graph.csc()
        dev = indptr.device
        n, nnz = indptr.shape[0] - 1, indices.shape[0]
        if b > n:
            raise GaeHipError(f"{who}: the block width {b} exceeds the {n} nodes of the graph")
        with _on_device(dev):
            if not (torch.equal(indptr, t_indptr) and torch.equal(indices, t_indices)):
                raise GaeHipError(f"{who}: the graph is not symmetric (its CSR differs from the CSR of its transpose); "
                                  "list every edge in both directions")
            f64 = dict(dtype=torch.float64, device=dev)
            s = torch.empty(n, **f64)
            blocks = [torch.empty(n, b, **f64) for _ in range(4)]
            G, H, T = (torch.empty(b, b, **f64) for _ in range(3))
            values, residuals = torch.empty(b, **f64), torch.empty(b, **f64)
            coef = torch.zeros(SPECTRAL_MAX_DEGREE + 1, 3, **f64)
            coef[0, 0] = 1.0
            status = torch.zeros(STATUS_WORDS, dtype=torch.int64, device=dev)
            ws = torch.empty(_ws_bytes("gae_spectral_workspace_bytes", n, nnz, b), dtype=torch.uint8, device=dev)
            vectors = torch.empty(n, k, **f64)
            embedding = torch.empty(n, k, dtype=torch.float32, device=dev)

            def product(yin, yprev, yout, row):
                _lib.call("gae_spectral_spmm", _ptr(indptr), _ptr(indices), n, nnz, _ptr(s), sigma, _ptr(yin), _ptr(yprev),
                          _ptr(yout), b, coef[row].data_ptr(), _ptr(status), _stream())

            def outer(V, AV):
                product(V, None, AV, 0)
                _lib.call("gae_spectral_gram", _ptr(V), _ptr(AV), n, b, _ptr(G), _ptr(H), 0, _ptr(ws), ws.numel(), _stream())
                _lib.call("gae_spectral_solve", _ptr(G), _ptr(H), b, kk, degree, _ptr(T), _ptr(values), _ptr(coef),
                          _ptr(status), _ptr(ws), ws.numel(), _stream())
                _lib.call("gae_spectral_rotate", _ptr(V), _ptr(AV), n, b, kk, _ptr(T), _ptr(values), tol, _ptr(residuals),
                          _ptr(status), _ptr(ws), ws.numel(), _stream())

            def run():
                _lib.call("gae_spectral_scale", _ptr(indptr), n, sigma, _ptr(s), _stream())
                V, AV, P, Q = blocks
                _lib.call("gae_spectral_init", _ptr(V), n, b, seed, _stream())
                it = 0
                while True:
                    it += 1
                    outer(V, AV)
                    if it % check_every == 0 or it == max_iter:
                        host = status.cpu()                                # the one read of a checked iteration
                        info, errors = int(host[0]), int(host[4])
                        if errors:
                            raise GaeHipError(f"{who}: the device reported error flags 0x{errors:x} (a CSR index outside the graph)")
                        if info > 0:
                            raise GaeHipError(f"{who}: the Gram matrix of the block lost rank at iteration {it} (Cholesky "
                                              f"pivot {info} of {b}); use a smaller degree or block")
                        if info < 0:
                            raise GaeHipError(f"{who}: the {b} x {b} eigensolver failed at iteration {it} (info = {info})")
                        if int(host[3]):
                            raise GaeHipError(f"{who}: {int(host[3])} residuals are not finite at iteration {it}")
                        if int(host[1]) >= kk or it == max_iter:
                            return V, it, int(host[2]), int(host[1]) >= kk
                    # the filter: V <- p_m(S) V by the three-term recurrence, coefficients from the device
                    prev, cur, free = None, V, [AV, P, Q]
                    for d in range(1, degree + 1):
                        nxt = free.pop()
                        product(cur, prev, nxt, d)
                        if prev is not None:
                            free.append(prev)
                        prev, cur = cur, nxt
                    rest = [t for t in blocks if t is not cur]
                    V, AV, P, Q = cur, rest[0], rest[1], rest[2]

            V, n_iter, n_spmm, converged = _timed(("spectral", n, nnz, b), run)
            first = 1 if drop_first else 0
            _lib.call("gae_spectral_finish", _ptr(V), n, b, first, k, _ptr(values), _ptr(s), _SCALINGS[scaling], _ptr(vectors),
                      _ptr(embedding), _ptr(ws), ws.numel(), _stream())
        return SpectralResult(embedding, vectors, values[first:first + k].clone(), residuals[first:first + k].clone(), n_iter,
                              n_spmm, converged, 0)
