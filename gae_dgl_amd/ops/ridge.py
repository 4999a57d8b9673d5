"""Ridge regression on a frozen feature with a k-fold CV lambda path (K25, gae_ridge_stats / gae_ridge_solve): the "GAE +
Ridge" row of the reference's chemistry table on the device.  One pass over ``X`` gives per-fold fp64 second moments
(the fp64 matrix core, no float atomics, the same bits run to run); every fold's fit, every fold's held-out error and
the final model follow from them in one more launch.  ``GAE.ridge_graphs``; ``python -m gae_dgl_amd.embed --ridge``.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import collections

import torch

from .. import _lib
from .._lib import GaeHipError
from ._base import _gpu, _on_device, _ptr, _stream, _timed, _ws_bytes
from ._heads import _CV_PATH, _choose, _fold_lists, _lambda_path, _rows, _targets

__all__ = ['RidgeResult', 'ridge', 'RIDGE_MAX_D', 'RIDGE_MAX_T', 'RIDGE_MAX_FOLDS', 'RIDGE_MAX_LAMBDAS', 'RIDGE_CHUNK_ROWS']

RIDGE_MAX_D, RIDGE_MAX_T, RIDGE_MAX_FOLDS, RIDGE_MAX_LAMBDAS = 128, 8, 32, 64
RIDGE_CHUNK_ROWS = _lib.RIDGE_CHUNK_ROWS
STATUS_WORDS = 4          # gae_ridge_status: int64 nonfinite_rows, errors, reserved[2]


class RidgeResult(collections.namedtuple("RidgeResult", [
        "coef", "intercept", "lam", "lambdas", "cv_rmse", "cv_r2", "cv_sse", "path_coef", "path_intercept", "info", "n_used",
        "fold_counts"])):
    """coef fp64 [t, d] (``torch.nn.Linear`` layout) and intercept fp64 [t] of the model fitted on all listed rows at the
    chosen ``lam``; lambdas fp64 [L]; cv_rmse / cv_r2 fp64 [L, t] from the SSE pooled over the folds (R2 against the SST
    of the listed rows about their overall mean); cv_sse fp64 [F, L, t]; path_coef fp64 [L, t, d] and path_intercept
    [L, t]: the all-rows model at every lambda; info int32 [F + 1, L] (gae_ridge_solve's; row F is the all-rows model);
    n_used listed rows; fold_counts int64 [F].  With ``folds=1`` there is no CV: the cv_* tables hold NaN."""
    __slots__ = ()

    def predict(self, X):
        """fp64 [n, t]: ``X @ coef^T + intercept`` by torch"""
        return X.double() @ self.coef.t() + self.intercept


def _options(lambdas, folds, fit_intercept, pivot):
    lambdas, folds = _lambda_path(lambdas, folds, RIDGE_MAX_LAMBDAS, _CV_PATH, RIDGE_MAX_FOLDS)
    if not isinstance(fit_intercept, bool):
        raise ValueError(f"fit_intercept: True or False, not {fit_intercept!r}")
    if not (pivot is None or isinstance(pivot, torch.Tensor) or pivot == "mean"):
        raise ValueError(f"pivot: 'mean', None or a [d + t] tensor, not {pivot!r}")
    return lambdas, folds


def ridge(X, y, lambdas=None, *, folds=5, fold=None, seed=0, fit_intercept=True, pivot="mean"):
    """``RidgeResult`` of ridge regression of ``y`` ([n] or [n, t], any float dtype, read as fp32) on the rows of ``X``
    [n, d] (fp32, on the GPU; read in place when the inner stride is 1), the penalty chosen by k-fold cross-validation
    among ``lambdas`` (default 10^-3 .. 10^3, 13 values): the lambda with the smallest mean over the targets of
    ``1 - cv_r2`` among those whose every model factorised, ties to the lower index.  ``fold``: an int tensor [n] with
    values in -1..folds-1 (-1: the row is left out, a test set for instance; such rows are never read); default: a
    permutation seeded by ``seed``, dealt round-robin.  An empty fold is a ValueError.  ``folds=1``: no CV, exactly one
    lambda.  The intercept is not penalised.  ``pivot``: "mean" (the fp32 column means of the listed rows), None (zeros)
    or a [d + t] tensor -- the moments are taken about it; the result does not depend on it mathematically.
    X is streamed once; the status block and the CV table are read back once.  1 <= d <= 128, 1 <= t <= 8, folds <= 32,
    <= 64 lambdas; a non-finite value in a listed row, or no lambda whose models all factorise, raises GaeHipError; there
    is no CPU fallback."""
    lambdas, F = _options(lambdas, folds, fit_intercept, pivot)
    with torch.no_grad():
        X, ldx, n, d = _rows(X, "ridge")
        dev = X.device
        Y, ldy, t = _targets(y, n, dev, "ridge")
        L, W = len(lambdas), 1 + d + t
        with _on_device(dev):
            nbytes = _ws_bytes("gae_ridge_workspace_bytes", n, d, t, F)     # shape errors before any other work
            rows, fold_ptr, counts = _fold_lists(fold, n, F, seed, dev)
            n_used = rows.shape[0]
            everything = n_used == n
            if isinstance(pivot, torch.Tensor):
                piv = _gpu(pivot, "ridge: pivot").detach().float().reshape(-1).contiguous()
                if piv.shape[0] != d + t or piv.device != dev:
                    raise GaeHipError(f"ridge: pivot must hold d + t = {d + t} values on {dev}")
            elif pivot == "mean":
                sel = rows.long()
                piv = torch.cat([(X if everything else X.index_select(0, sel)).mean(0),
                                 (Y if everything else Y.index_select(0, sel)).mean(0)]).contiguous()
            else:
                piv = None
            lam_dev = torch.tensor(lambdas, dtype=torch.float64, device=dev)
            stats = torch.empty(F, W * (W + 1) // 2, dtype=torch.float64, device=dev)
            status = torch.zeros(STATUS_WORDS, dtype=torch.int64, device=dev)
            coef = torch.empty(F + 1, L, t, d, dtype=torch.float64, device=dev)
            icpt = torch.empty(F + 1, L, t, dtype=torch.float64, device=dev)
            sse = torch.empty(F, L, t, dtype=torch.float64, device=dev)
            info = torch.empty(F + 1, L, dtype=torch.int32, device=dev)
            ws = torch.empty(int(_lib.load().gae_ridge_workspace_bytes(n_used, d, t, F)), dtype=torch.uint8, device=dev)
            flags = 0 if fit_intercept else _lib.RIDGE_NO_INTERCEPT

            def launch():
                _lib.call("gae_ridge_stats", _ptr(X), ldx, _ptr(Y), ldy, n, d, t, _ptr(piv), _ptr(rows), n_used,
                          _ptr(fold_ptr), F, _ptr(stats), _ptr(status), _ptr(ws), ws.numel(), _stream())
                _lib.call("gae_ridge_solve", _ptr(stats), d, t, F, _ptr(piv), _ptr(lam_dev), L, flags, _ptr(coef),
                          _ptr(icpt), _ptr(sse), _ptr(info), _ptr(status), _stream())
            _timed(("ridge", n_used, d, t, F, L), launch)
            # SST of the listed rows about their overall mean, from the moments: S_yy - S_y^2 / c per target
            total = stats.sum(0)
            iy = [(1 + d + j) * W - (1 + d + j) * (d + j) // 2 for j in range(t)]
            sst = total[iy] - total[1 + d:1 + d + t] ** 2 / total[0]
            host = torch.cat([status.double(), info.double().reshape(-1), sse.reshape(-1), sst]).cpu()   # the one read
        bad, errors = int(host[0]), int(host[1])
        if errors:
            raise GaeHipError(f"ridge: the device reported error flags 0x{errors:x} (fold lists or lambdas)")
        if bad:
            raise GaeHipError(f"ridge: {bad} of the {n_used} listed rows hold non-finite values")
        info_h = host[STATUS_WORDS:STATUS_WORDS + (F + 1) * L].reshape(F + 1, L)
        sse_h = host[STATUS_WORDS + (F + 1) * L:-t].reshape(F, L, t)
        sst_h = host[-t:]
        pooled = sse_h.sum(0)                                          # [L, t]
        cv_rmse = torch.sqrt(pooled.clamp_min(0.0) / n_used)           # (an SSE of zero may come out as -1e-20)
        cv_r2 = 1.0 - pooled / sst_h
        if F == 1:
            ok = [bool(info_h[1, 0] == 0)]
            score = [0.0]
        else:
            ok = [bool((info_h[:, l] == 0).all()) for l in range(L)]
            score = [float((1.0 - cv_r2[l]).mean()) for l in range(L)]
        best = _choose(ok, score)
        if best < 0:
            raise GaeHipError(f"ridge: none of the {L} lambdas gave a model for every fold "
                              f"({sum(1 for v in ok if not v)} failed to factorise; info = {info_h.int().tolist()})")
    return RidgeResult(coef[F, best], icpt[F, best], lambdas[best], lam_dev, cv_rmse.to(dev), cv_r2.to(dev), sse, coef[F],
                       icpt[F], info, n_used, counts)
