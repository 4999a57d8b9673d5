"""Principal components of a frozen feature (K31, gae_pca_solve / gae_pca_transform): the explained-variance spectrum, a
linear projection to k dimensions, whitening.  ``gae_ridge_stats`` (K25) gives the exact-order fp64 second moments of the
listed rows in one pass; one block diagonalises the centred d x d matrix by a cyclic Jacobi method in fp64 (every rotation
a stated sequence of operations: the same bits run to run, no rocSOLVER call, no host round trip); one more pass
projects.  ``GAE.pca_nodes`` / ``GAE.pca_graphs``; ``ops.tsne(init="pca")``; ``python -m gae_dgl_amd.embed --pca``.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import collections

import torch

import gae_dgl_amd.ops as _ops
from .. import _lib
from .._lib import GaeHipError
from ._base import _gpu, _on_device, _ptr, _stream, _timed, _ws_bytes
from ._heads import _listed, _rows

__all__ = ['PCAResult', 'pca', 'pca_transform', 'PCA_MAX_D', 'PCA_MAX_SWEEPS']

PCA_MAX_D, PCA_MAX_SWEEPS = _lib.PCA_MAX_D, _lib.PCA_MAX_SWEEPS
RIDGE_STATUS_WORDS = 4    # gae_ridge_status
STATUS_WORDS = _lib.PCA_STATUS_WORDS


class PCAResult(collections.namedtuple("PCAResult", [
        "components", "explained_variance", "explained_variance_ratio", "singular_values", "mean", "n_used", "n_sweeps",
        "info", "whiten"])):
    """components fp64 [k, d] (unit rows; the entry of largest magnitude of each is positive); explained_variance fp64
    [k] (the eigenvalues of the n - 1 covariance, descending, as computed); explained_variance_ratio [k] (each over the
    sum of ALL d eigenvalues); singular_values [k] = sqrt(lambda (n_used - 1)); mean fp64 [d]; n_used listed rows;
    n_sweeps Jacobi sweeps; info 0; whiten: what ``transform`` does."""
    __slots__ = ()

    def transform(self, X, rows=None):
        """fp32 [n or len(rows), k]: the scores of the rows of ``X`` (``ops.pca_transform``)"""
        return _ops.pca_transform(X, self.mean, self.components, self.explained_variance, self.whiten, rows=rows)

    def inverse_transform(self, Z):
        """fp64 [n, d]: ``Z @ components + mean`` by torch (whitened scores are scaled back first)"""
        Z = Z.double()
        if self.whiten:
            Z = Z * torch.sqrt(self.explained_variance.clamp_min(0.0))
        return Z @ self.components + self.mean


def pca(X, n_components=None, *, rows=None, whiten=False, pivot="mean"):
    """``PCAResult`` of the rows of ``X`` [n, d] (fp32, on the GPU; read in place when the inner stride is 1): the
    ``n_components`` (default: all d) leading eigenpairs of the n - 1 covariance of the listed rows.  ``rows``: an int
    tensor of row ids or a bool mask [n]; rows outside it are never read.  ``pivot``: "mean" (the fp32 column means of
    the listed rows), None (zeros) or a [d] tensor -- the moments are taken about it; the result does not depend on it
    mathematically, a pivot near the means keeps them small.  ``whiten``: ``transform`` divides every score by the
    square root of its variance.  X is streamed once; the host reads the status once.  1 <= d <= 128; fewer than two
    listed rows is a ValueError; a non-finite value in a listed row, or a solver that does not converge, raises
    GaeHipError; there is no CPU fallback."""
    if not isinstance(whiten, bool):
        raise ValueError(f"whiten: True or False, not {whiten!r}")
    if not (pivot is None or isinstance(pivot, torch.Tensor) or pivot == "mean"):
        raise ValueError(f"pivot: 'mean', None or a [d] tensor, not {pivot!r}")
    with torch.no_grad():
        X, ldx, n, d = _rows(X, "pca")
        dev = X.device
        if not 1 <= d <= PCA_MAX_D:
            raise GaeHipError(f"pca: d = {d} outside 1..{PCA_MAX_D} (there is no fallback for wider features)")
        k = d if n_components is None else n_components
        if isinstance(k, bool) or int(k) != k or not 1 <= k <= d:
            raise GaeHipError(f"pca: n_components = {n_components!r} outside 1..d = {d}")
        k = int(k)
        with _on_device(dev):
            listed = _listed(rows, n, dev, "pca")
            n_used = n if listed is None else listed.shape[0]
            if n_used < 2:
                raise ValueError(f"pca: {n_used} listed rows; a covariance needs at least two")
            W = d + 2
            if isinstance(pivot, torch.Tensor):
                px = _gpu(pivot, "pca: pivot").detach().float().reshape(-1)
                if px.shape[0] != d or px.device != dev:
                    raise GaeHipError(f"pca: pivot must hold d = {d} values on {dev}")
            elif pivot == "mean":
                px = (X if listed is None else X.index_select(0, listed.long())).mean(0)
            else:
                px = torch.zeros(d, dtype=torch.float32, device=dev)
            piv = torch.cat([px, px[:1]]).contiguous()                     # the target is column 0 of X
            fold_ptr = torch.tensor([0, n_used], dtype=torch.int32, device=dev)
            stats = torch.empty(W * (W + 1) // 2, dtype=torch.float64, device=dev)
            rstatus = torch.zeros(RIDGE_STATUS_WORDS, dtype=torch.int64, device=dev)
            status = torch.zeros(STATUS_WORDS, dtype=torch.int64, device=dev)
            mean = torch.empty(d, dtype=torch.float64, device=dev)
            values = torch.empty(k, dtype=torch.float64, device=dev)
            comps = torch.empty(k, d, dtype=torch.float64, device=dev)
            ws = torch.empty(max(_ws_bytes("gae_ridge_workspace_bytes", n_used, d, 1, 1), _ws_bytes("gae_pca_workspace_bytes", d)),
                             dtype=torch.uint8, device=dev)

            def launch():
                _lib.call("gae_ridge_stats", _ptr(X), ldx, _ptr(X), ldx, n, d, 1, _ptr(piv), _ptr(listed), n_used,
                          _ptr(fold_ptr), 1, _ptr(stats), _ptr(rstatus), _ptr(ws), ws.numel(), _stream())
                _lib.call("gae_pca_solve", _ptr(stats), d, 1, _ptr(piv), n_used, k, 0, _ptr(mean), _ptr(values), _ptr(comps),
                          _ptr(status), _ptr(ws), ws.numel(), _stream())
            _timed(("pca", n_used, d, k), launch)
            host = torch.cat([rstatus, status]).cpu()                      # the one read
        bad, errors = int(host[0]), int(host[1])
        info, sweeps = int(host[RIDGE_STATUS_WORDS]), int(host[RIDGE_STATUS_WORDS + 1])
        if errors:
            raise GaeHipError(f"pca: the device reported error flags 0x{errors:x} (row list)")
        if bad:
            raise GaeHipError(f"pca: {bad} of the {n_used} listed rows hold non-finite values")
        if info != 0:
            raise GaeHipError(f"pca: the eigensolver did not converge (info = {info} after {sweeps} sweeps of at most "
                              f"{PCA_MAX_SWEEPS})")
        total = status[7:8].view(torch.float64)                            # total_variance, stays on the device
        return PCAResult(comps, values, values / total, torch.sqrt((values * float(n_used - 1)).clamp_min(0.0)), mean, n_used,
                         sweeps, info, whiten)


def pca_transform(X, mean, components, values=None, whiten=False, *, rows=None, status=None):
    """fp32 [n or len(rows), k]: ``Z[i][c] = sum_j (x_ij - mean_j) components[c][j]`` of the (listed) rows of ``X`` [n, d]
    by gae_pca_transform: mean and components rounded to fp32 once, one fp32 subtraction, one fp32 fma chain over j
    ascending; ``whiten`` multiplies by the fp32 rounding of 1 / sqrt(values[c]) (a value that is not > 0 gives score 0).
    A listed row that holds a non-finite value gives a NaN row.  ``status``: an int64 [8] device tensor that receives the
    counts (gae_pca_status; None: not reported).  No host synchronisation."""
    with torch.no_grad():
        X, ldx, n, d = _rows(X, "pca_transform")
        dev = X.device
        mean = _gpu(mean, "pca_transform: mean").detach().double().reshape(-1).contiguous()
        comps = _gpu(components, "pca_transform: components").detach().double().contiguous()
        if comps.dim() != 2 or comps.shape[1] != d or mean.shape[0] != d or comps.device != dev or mean.device != dev:
            raise GaeHipError(f"pca_transform: mean [{d}] and components [k, {d}] on {dev}, got {tuple(mean.shape)} and "
                              f"{tuple(comps.shape)}")
        k = comps.shape[0]
        if whiten:
            if values is None:
                raise GaeHipError("pca_transform: whiten=True needs the variances (values)")
            values = _gpu(values, "pca_transform: values").detach().double().reshape(-1).contiguous()
            if values.shape[0] != k or values.device != dev:
                raise GaeHipError(f"pca_transform: values must hold k = {k} variances on {dev}")
        else:
            values = None
        with _on_device(dev):
            listed = _listed(rows, n, dev, "pca_transform")
            n_rows = n if listed is None else listed.shape[0]
            if status is None:
                status = torch.zeros(STATUS_WORDS, dtype=torch.int64, device=dev)
            Z = torch.empty(n_rows, k, dtype=torch.float32, device=dev)

            def launch():
                _lib.call("gae_pca_transform", _ptr(X), ldx, n, d, _ptr(listed), n_rows, _ptr(mean), _ptr(comps), _ptr(values),
                          k, _lib.PCA_WHITEN if whiten else 0, _ptr(Z), max(k, 1), _ptr(status), _stream())
            _timed(("pca_transform", n_rows, d, k), launch)
    return Z
