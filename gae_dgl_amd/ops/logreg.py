"""Multinomial logistic regression on a frozen feature with a k-fold CV lambda path (K28, gae_logreg_*): the standard
protocol for judging an unsupervised embedding -- freeze it, fit a softmax classifier on the labelled rows, report the
held-out accuracy -- on the device.  Every (fold model or all-rows model) x lambda of a call runs in the same launches:
fp32 matrix-core passes, fp64 moments and updates, no float atomics, the same bits run to run.
``GAE.classify_nodes``, ``GAE.logreg_graphs``; ``python -m gae_dgl_amd.embed --logreg``; ``train_transductive --classify``.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import collections
import math

import torch

import gae_dgl_amd.ops as _ops
from .. import _lib
from .._lib import GaeHipError
from ._base import _gpu, _on_device, _ptr, _stream, _timed, _ws_bytes
from ._heads import _CV_PATH, _choose, _default_fold, _fold_arg, _fold_lists, _lambda_path, _rows, _status_arg

__all__ = ['LogRegResult', 'logreg', 'logreg_predict', 'LOGREG_MAX_D', 'LOGREG_MAX_CLASSES', 'LOGREG_MAX_FOLDS',
           'LOGREG_MAX_LAMBDAS', 'LOGREG_CHUNK_ROWS', 'LOGREG_SLAB_CHUNKS']

LOGREG_MAX_D, LOGREG_MAX_CLASSES, LOGREG_MAX_FOLDS, LOGREG_MAX_LAMBDAS = 128, 32, 32, 64
LOGREG_CHUNK_ROWS, LOGREG_SLAB_CHUNKS = _lib.LOGREG_CHUNK_ROWS, _lib.LOGREG_SLAB_CHUNKS
STATUS_WORDS = 4          # gae_logreg_status: int64 active_models, nonfinite_rows, errors, reserved
PARTIAL_BYTES = 256 << 20  # the default model_batch keeps one launch's partials below this


class LogRegResult(collections.namedtuple("LogRegResult", [
        "coef", "intercept", "lam", "lambdas", "cv_logloss", "cv_accuracy", "cv_nll", "cv_correct", "path_coef",
        "path_intercept", "info", "n_iter", "converged", "train_logloss", "n_used", "fold_counts", "class_counts", "pivot", "fold_coef",
        "fold_intercept"])):
    """coef fp64 [c, d] (``torch.nn.Linear`` layout) and intercept fp64 [c] of the model fitted on all listed rows at the
    chosen ``lam``; lambdas fp64 [L]; cv_logloss / cv_accuracy fp64 [L]: the held-out negative log-likelihood per row and
    the held-out accuracy, pooled over the folds; cv_nll fp64 [F, L] and cv_correct int64 [F, L]: fold model f on its own
    fold; path_coef fp64 [L, c, d] and path_intercept [L, c]: the all-rows model at every lambda; info / n_iter /
    converged int32 [F + 1, L] (row F is the all-rows model; info as gae_logreg_factor's); train_logloss: the all-rows
    model's negative log-likelihood per listed row at ``lam``; n_used listed rows; fold_counts int64 [F]; class_counts
    int64 [c]; pivot fp32 [d]; fold_coef fp64 [F, L, c, d] and fold_intercept [F, L, c]: the fold
    models, the ones cv_nll and cv_correct were taken with.  With ``folds=1`` there is no CV: the cv_* tables hold NaN / 0.

    W starts at 0 and every update sums to zero over the classes, so the parameters sum to (about) zero over the classes:
    the minimum-norm representative of the shift-invariant intercepts."""
    __slots__ = ()

    def predict(self, X):
        """int32 [n]: the arg-max class of every row of ``X`` (ops.logreg_predict); -1 for a row with a non-finite value"""
        return _ops.logreg_predict(X, self.coef, self.intercept, self.pivot)

    def predict_proba(self, X):
        """fp32 [n, c]: the class probabilities of every row of ``X`` (ops.logreg_predict); NaN for a non-finite row"""
        return _ops.logreg_predict(X, self.coef, self.intercept, self.pivot, proba=True)[1]

    def to_torch(self):
        """``torch.nn.Linear(d, c)`` (fp32, on the result's device) whose softmax is ``predict_proba``"""
        c, d = self.coef.shape
        lin = torch.nn.Linear(d, c, device=self.coef.device)
        with torch.no_grad():
            lin.weight.copy_(self.coef.float())
            lin.bias.copy_(self.intercept.float())
        return lin


def _options(X, y, lambdas, folds, n_classes, max_iter, tol, check_every, model_batch):
    """the checks that need no device: (lambdas, F, c)"""
    lambdas, folds = _lambda_path(lambdas, folds, LOGREG_MAX_LAMBDAS, [1.0] if folds == 1 else _CV_PATH, LOGREG_MAX_FOLDS)
    for name, v in (("max_iter", max_iter), ("check_every", check_every)):
        if isinstance(v, bool) or int(v) != v or not 1 <= v < 2 ** 31:
            raise ValueError(f"{name}: a positive integer, not {v!r}")
    if not (isinstance(tol, (int, float)) and tol >= 0.0 and math.isfinite(tol)):
        raise ValueError(f"tol: a finite number >= 0, not {tol!r}")
    if model_batch is not None and (isinstance(model_batch, bool) or int(model_batch) != model_batch or model_batch < 1):
        raise ValueError(f"model_batch: None or a positive integer, not {model_batch!r}")
    if not isinstance(X, torch.Tensor) or X.dim() != 2:
        raise ValueError(f"X: a 2-D tensor, not {getattr(X, 'shape', type(X))}")
    n, d = X.shape
    if not 1 <= d <= LOGREG_MAX_D:
        raise ValueError(f"X: d = {d} outside 1..{LOGREG_MAX_D}")
    if not isinstance(y, torch.Tensor) or y.dtype.is_floating_point or y.dtype == torch.bool or y.dim() != 1 \
            or y.shape[0] != n:
        raise ValueError(f"y: an int tensor [{n}] of classes (-1 = unlabelled)")
    lo, hi = (int(y.min()), int(y.max())) if n else (0, -1)
    if n_classes is None:
        c = hi + 1
    elif isinstance(n_classes, bool) or int(n_classes) != n_classes:
        raise ValueError(f"n_classes: an integer in 2..{LOGREG_MAX_CLASSES}, not {n_classes!r}")
    else:
        c = int(n_classes)
    if not 2 <= c <= LOGREG_MAX_CLASSES:
        raise ValueError(f"the number of classes c = {c} lies outside 2..{LOGREG_MAX_CLASSES}")
    if lo < -1 or hi >= c:
        raise ValueError(f"y: values in -1..{c - 1} (-1 = unlabelled), got {lo}..{hi}")
    return lambdas, folds, c


def logreg(X, y, lambdas=None, *, folds=5, fold=None, seed=0, n_classes=None, max_iter=1000, tol=1e-4, check_every=8,
           model_batch=None):
    """``LogRegResult`` of multinomial (softmax) logistic regression with an L2 penalty of the classes ``y`` (an int
    tensor [n] with values in -1..c-1; -1: unlabelled) on the rows of ``X`` [n, d] (fp32, on the GPU; read in place when
    the inner stride is 1).  Per model J(b, W) = sum_i -log softmax(b + W x_i)[y_i] + (lambda / 2) sum_k |w_k|^2 over its
    training rows -- sklearn's ``C = 1 / lambda``, the intercepts not penalised.  The penalty is chosen by k-fold
    cross-validation among ``lambdas`` (default 10^-3 .. 10^3, 13 values): the smallest pooled held-out log-loss among the
    lambdas whose every model factorised and stayed finite, ties to the lower index.  ``fold``: an int tensor [n] with
    values in -1..folds-1 (-1: left out, a test set for instance); default: a permutation seeded by ``seed``, dealt
    round-robin.  A row with ``y = -1`` or ``fold = -1`` is not listed and never read.  An empty fold is a ValueError.
    ``folds=1``: a plain fit with exactly one lambda (default 1).  ``n_classes``: c when the largest label does not say it.

    The solver is first order in the metric of a fixed majoriser (Boehning's bound, factorised once per model), Nesterov
    accelerated with gradient restart; every fold x lambda model runs in the same launches.  A model stops when
    max|dV| <= ``tol`` max(1, max|W|) and is frozen from then on, so no result depends on the other models, on
    ``check_every`` (passes between two reads of the 32-byte status block) or on ``model_batch`` (models per launch;
    default: as many as keep the partial sums below 256 MB).  Reaching ``max_iter`` is not an error: ``converged`` says so.

    The returned parameters sum to (about) zero over the classes -- W starts at 0 and every update sums to zero over the
    classes: the minimum-norm representative of the shift-invariant intercepts.

    1 <= d <= 128, 2 <= c <= 32, folds <= 32, <= 64 lambdas; a non-finite feature in a listed row, or no lambda whose
    models all factorised and stayed finite, raises GaeHipError; there is no CPU fallback."""
    lambdas, F, c = _options(X, y, lambdas, folds, n_classes, max_iter, tol, check_every, model_batch)
    n, d = X.shape
    if fold is None:
        fold = _default_fold(n, F, seed).to(y.device)
    else:
        _fold_arg(fold, n, F)
    fold = fold.to(y.device).long()
    fold = torch.where(y < 0, torch.full_like(fold, -1), fold)          # an unlabelled row is not listed
    rows, fold_ptr, counts = _fold_lists(fold, n, F, seed, y.device)    # (an empty fold: ValueError)
    L, M = len(lambdas), (F + 1) * len(lambdas)
    with torch.no_grad():
        X, ldx, n, d = _rows(X, "logreg")
        dev = X.device
        y = _gpu(y, "logreg: y").detach()
        if y.device != dev:
            raise GaeHipError(f"logreg: y must be on {dev}, not on {y.device}")
        with _on_device(dev):
            n_used = rows.shape[0]
            slabs = -(-(-(-n_used // LOGREG_CHUNK_ROWS) + F) // LOGREG_SLAB_CHUNKS)
            batch = max(1, min(M, PARTIAL_BYTES // (slabs * c * (d + 1) * 4))) if model_batch is None else min(int(model_batch), M)
            nbytes = _ws_bytes("gae_logreg_workspace_bytes", n_used, d, c, F, L, batch)
            rows, fold_ptr = rows.to(dev), fold_ptr.to(dev)
            sel = rows.long()
            y32 = y.to(torch.int32).contiguous()
            piv = X.index_select(0, sel).mean(0).contiguous()           # the listed rows in list order: never another row
            class_counts = torch.bincount(y.index_select(0, sel).long(), minlength=c)
            ycol = y32.float().reshape(n, 1)                            # gae_ridge_stats' one target; its moments are ignored
            piv_r = torch.cat([piv, piv.new_zeros(1)])
            lam_dev = torch.tensor(lambdas, dtype=torch.float64, device=dev)
            Wr = d + 2
            stats = torch.empty(F, Wr * (Wr + 1) // 2, dtype=torch.float64, device=dev)
            rstatus = torch.zeros(4, dtype=torch.int64, device=dev)
            status = torch.zeros(STATUS_WORDS, dtype=torch.int64, device=dev)
            coef = torch.empty(F + 1, L, c, d, dtype=torch.float64, device=dev)
            icpt = torch.empty(F + 1, L, c, dtype=torch.float64, device=dev)
            info = torch.empty(F + 1, L, dtype=torch.int32, device=dev)
            n_iter = torch.empty(F + 1, L, dtype=torch.int32, device=dev)
            conv = torch.empty(F + 1, L, dtype=torch.int32, device=dev)
            nll = torch.empty(F + 1, L, dtype=torch.float64, device=dev)
            correct = torch.empty(F + 1, L, dtype=torch.int64, device=dev)
            rws = torch.empty(int(_lib.load().gae_ridge_workspace_bytes(n_used, d, 1, F)), dtype=torch.uint8, device=dev)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            cuts = [(lo, min(batch, M - lo)) for lo in range(0, M, batch)]

            def run_pass(lo, cnt, flags):
                _lib.call("gae_logreg_pass", _ptr(X), ldx, _ptr(y32), n, d, c, _ptr(piv), _ptr(rows), n_used, _ptr(fold_ptr),
                          F, L, batch, lo, cnt, flags, _ptr(nll), _ptr(correct), _ptr(status), _ptr(ws), nbytes, _stream())

            def launch():
                _lib.call("gae_ridge_stats", _ptr(X), ldx, _ptr(ycol), 1, n, d, 1, _ptr(piv_r), _ptr(rows), n_used,
                          _ptr(fold_ptr), F, _ptr(stats), _ptr(rstatus), _ptr(rws), rws.numel(), _stream())
                _lib.call("gae_logreg_factor", _ptr(stats), d, c, F, _ptr(lam_dev), L, n_used, batch, _ptr(coef), _ptr(icpt),
                          _ptr(info), _ptr(n_iter), _ptr(conv), _ptr(status), _ptr(ws), nbytes, _stream())
                for it in range(1, int(max_iter) + 1):
                    for lo, cnt in cuts:
                        run_pass(lo, cnt, 0)
                        _lib.call("gae_logreg_update", d, c, F, _ptr(lam_dev), L, n_used, batch, lo, cnt, it, int(max_iter),
                                  float(tol), _ptr(piv), _ptr(coef), _ptr(icpt), _ptr(info), _ptr(n_iter), _ptr(conv),
                                  _ptr(status), _ptr(ws), nbytes, _stream())
                    if it % int(check_every) == 0 and it < max_iter and int(status[0]) == 0:   # the 32-byte read
                        break
                for lo, cnt in cuts:
                    run_pass(lo, cnt, _lib.LOGREG_EVAL)
            _timed(("logreg", n_used, d, c, F, L), launch)
            host = torch.cat([rstatus.double(), status.double(), info.double().reshape(-1), nll.reshape(-1),
                              correct.double().reshape(-1)]).cpu()      # the one read of the tables
        bad, rerr, errors = int(host[0]), int(host[1]), int(host[6])
        if rerr or errors & ~_lib.LOGREG_ERR_NONFINITE:
            raise GaeHipError(f"logreg: the device reported error flags 0x{rerr:x} / 0x{errors:x} (fold lists, lambdas or labels)")
        if bad:
            raise GaeHipError(f"logreg: {bad} of the {n_used} listed rows hold non-finite values")
        info_h = host[8:8 + M].reshape(F + 1, L)
        nll_h = host[8 + M:8 + 2 * M].reshape(F + 1, L)
        cor_h = host[8 + 2 * M:].reshape(F + 1, L)
        if F == 1:
            ok = [bool(info_h[1, 0] == 0) and math.isfinite(float(nll_h[1, 0]))]
            score = [0.0]
            cv_logloss = torch.full((L,), float("nan"), dtype=torch.float64)
            cv_acc = torch.full((L,), float("nan"), dtype=torch.float64)
        else:
            cv_logloss = nll_h[:F].sum(0) / n_used
            cv_acc = cor_h[:F].sum(0) / n_used
            ok = [bool((info_h[:, l] == 0).all()) and bool(torch.isfinite(nll_h[:, l]).all()) for l in range(L)]
            score = [float(v) for v in cv_logloss]
        best = _choose(ok, score)
        if best < 0:
            raise GaeHipError(f"logreg: none of the {L} lambdas gave a model for every fold that factorised and stayed "
                              f"finite (info = {info_h.int().tolist()})")
        if F == 1:
            cv_nll = torch.full((F, L), float("nan"), dtype=torch.float64, device=dev)
            cv_correct = torch.zeros(F, L, dtype=torch.int64, device=dev)
        else:
            cv_nll, cv_correct = nll[:F], correct[:F]
    return LogRegResult(coef[F, best], icpt[F, best], lambdas[best], lam_dev, cv_logloss.to(dev), cv_acc.to(dev), cv_nll,
                        cv_correct, coef[F], icpt[F], info, n_iter, conv, float(nll_h[F, best]) / n_used, n_used, counts,
                        class_counts, piv, coef[:F], icpt[:F])


def logreg_predict(X, coef, intercept, pivot=None, *, proba=False, status=None):
    """int32 [n]: the arg-max class (ties to the lower class) of every row of ``X`` [n, d] (fp32, on the GPU, any row
    stride) under the softmax model ``coef`` [c, d], ``intercept`` [c] (read as fp64), through the fit's own product and
    softmax code about ``pivot`` (fp32 [d] or None).  ``proba=True``: (labels, fp32 [n, c] probabilities).  A row holding
    a non-finite feature gets -1 / NaN and is counted in ``status`` (an int64 [4] device tensor the caller zeroed: word 1
    counts such rows; None: not reported).  No host synchronisation."""
    with torch.no_grad():
        X, ldx, n, d = _rows(X, "logreg_predict")
        dev = X.device
        coef = _gpu(coef, "logreg_predict: coef").detach().double().contiguous()
        intercept = _gpu(intercept, "logreg_predict: intercept").detach().double().contiguous()
        if coef.dim() != 2 or coef.shape[1] != d or intercept.shape != coef.shape[:1] or coef.device != dev \
                or intercept.device != dev:
            raise GaeHipError(f"logreg_predict: coef [c, {d}] and intercept [c] on {dev} expected, got {tuple(coef.shape)} "
                              f"and {tuple(intercept.shape)}")
        c = coef.shape[0]
        if pivot is not None:
            pivot = _gpu(pivot, "logreg_predict: pivot").detach().float().reshape(-1).contiguous()
            if pivot.shape[0] != d or pivot.device != dev:
                raise GaeHipError(f"logreg_predict: pivot must hold d = {d} values on {dev}")
        status = _status_arg(status, STATUS_WORDS, dev, "logreg_predict")
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        P = torch.empty(n, c, dtype=torch.float32, device=dev) if proba else None
        with _on_device(dev):
            _lib.call("gae_logreg_predict", _ptr(X), ldx, n, d, c, _ptr(coef), _ptr(intercept), _ptr(pivot), _ptr(labels),
                      _ptr(P), c, _ptr(status), _stream())
    return (labels, P) if proba else labels
