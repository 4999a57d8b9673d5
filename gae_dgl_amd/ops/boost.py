"""Second-order histogram gradient boosting on a frozen feature (K30, gae_boost_fit / gae_boost_predict): XGBoost's
objective on integer histograms, for regression ("squared") and binary classification ("logistic").  Every fold model and
every (learning rate, lambda) configuration of a call trains side by side in the same launches; the number of rounds and
the configuration are chosen by the pooled held-out loss after every round -- early stopping by cross-validation with no
further training.  Every accumulated quantity is an integer and every floating-point step a stated fp64 operation, so
tests/boost_ref.py restates a fit bit for bit.  ``GAE.boost_graphs``; ``python -m gae_dgl_amd.embed --boost``.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import collections
import ctypes
import math

import torch

import gae_dgl_amd.ops as _ops
from .. import _lib
from .._lib import GaeHipError
from ._base import _gpu, _on_device, _ptr, _stream, _timed, _ws_bytes
from ._heads import (_check_max_bins, _check_max_features, _check_min_samples_leaf, _check_seed, _default_fold, _edges,
                     _fold_arg, _rows, _status_arg, _whole)

__all__ = ['BoostResult', 'boost', 'boost_predict', 'BOOST_MAX_D', 'BOOST_MAX_BINS', 'BOOST_MAX_DEPTH', 'BOOST_MAX_ROUNDS',
           'BOOST_MAX_MODELS']

BOOST_MAX_D, BOOST_MAX_BINS, BOOST_MAX_DEPTH, BOOST_MAX_ROUNDS, BOOST_MAX_MODELS = 256, 256, 8, 4096, 256
OBJECTIVES = {"squared": _lib.BOOST_SQUARED, "logistic": _lib.BOOST_LOGISTIC}
STATUS_WORDS = 4          # gae_forest_status: int64 nonfinite, errors, reserved[2]


class BoostResult(collections.namedtuple("BoostResult", [
        "feature", "threshold_bin", "threshold", "left", "count", "value", "gain", "n_nodes", "base_score", "edges",
        "n_edges", "lr", "lam", "best_round", "best_cfg", "cv_curve", "cv_rmse", "cv_r2", "cv_logloss", "cv_accuracy",
        "importances", "info", "train_score", "objective", "n_used", "oof_score"])):
    """The all-rows model of the chosen configuration as node tables [R, M] over all R = n_rounds rounds, M =
    2^(max_depth + 1) - 1, fields as ``ForestResult``'s: feature int32 (-1 marks a leaf), threshold_bin int32, threshold
    fp32 (a row goes left iff x[feature] <= threshold), left int32 (the right child is left + 1), count int32, value fp64
    (the weight -lr G / (H + lambda) of EVERY node, the learning rate applied), gain fp64; n_nodes int32 [R].  base_score
    (a float): where every score starts; edges fp32 [d, max_bins - 1] / n_edges int32 [d]; lr, lam: the chosen pair,
    configuration best_cfg of ``learning_rates x lambdas`` (row-major); best_round: the number of trees ``predict`` uses;
    cv_curve fp64 [n_cfg, R]: the held-out loss per row (squared error or log-loss) pooled over the folds, with r + 1 trees
    at index r; cv_rmse / cv_r2 ("squared") or cv_logloss / cv_accuracy ("logistic") at the chosen point, NaN for the
    other objective; importances fp64 [d]: the gain per feature over the best_round trees, normalised to 1; info int32
    [n_cfg]: 1 where a model of the configuration left the fixed-point frame or went non-finite; train_score fp64
    [n_used]: the fit's final raw score of the listed rows, all R trees; oof_score fp64 [n_used] (``oof=True``; else None):
    every listed row's raw score under the model that held it out, with best_round trees.  With ``folds=1`` there is no
    CV: cv_* hold NaN and best_round = n_rounds."""
    __slots__ = ()

    def predict(self, X, n_rounds=None):
        """fp64 [m]: the raw score (the mean for "squared", the log-odds for "logistic") with ``n_rounds`` trees (None:
        best_round)"""
        return _ops.boost_predict(self, X, n_rounds=n_rounds)

    def predict_proba(self, X, n_rounds=None):
        """fp64 [m]: P(y = 1) of a "logistic" model"""
        if self.objective != "logistic":
            raise ValueError('predict_proba needs objective="logistic"')
        return torch.sigmoid(_ops.boost_predict(self, X, n_rounds=n_rounds))


def _values(v, name):
    if isinstance(v, torch.Tensor):
        v = v.detach().double().cpu().reshape(-1).tolist()
    else:
        v = [float(x) for x in (v if hasattr(v, "__iter__") else [v])]
    if not v:
        raise ValueError(f"{name}: at least one value")
    return v


def _options(X, y, objective, n_rounds, max_depth, learning_rates, lambdas, min_child_weight, min_samples_leaf, min_gain,
             max_features, max_bins, folds, seed, check_every):
    """the checks that need no device: (learning rates, lambdas, F)"""
    if objective not in OBJECTIVES:
        raise ValueError(f'objective: "squared" or "logistic", not {objective!r}')
    if not _whole(n_rounds) or not 1 <= n_rounds <= BOOST_MAX_ROUNDS:
        raise ValueError(f"n_rounds: an integer in 1..{BOOST_MAX_ROUNDS}, not {n_rounds!r}")
    if not _whole(max_depth) or not 1 <= max_depth <= BOOST_MAX_DEPTH:
        raise ValueError(f"max_depth: an integer in 1..{BOOST_MAX_DEPTH}, not {max_depth!r}")
    _check_max_bins(max_bins, BOOST_MAX_BINS)
    _check_min_samples_leaf(min_samples_leaf)
    if not _whole(check_every) or check_every < 1:
        raise ValueError(f"check_every: a positive integer, not {check_every!r}")
    _check_seed(seed)
    if not _whole(folds) or not 1 <= folds < BOOST_MAX_MODELS:
        raise ValueError(f"folds: an integer in 1..{BOOST_MAX_MODELS - 1}, not {folds!r}")
    _check_max_features(max_features)
    for name, v in (("min_child_weight", min_child_weight), ("min_gain", min_gain)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not (v >= 0.0 and math.isfinite(v)):
            raise ValueError(f"{name}: a finite number >= 0, not {v!r}")
    lrs, lams = _values(learning_rates, "learning_rates"), _values(lambdas, "lambdas")
    if not all(0.0 < v <= 1.0 for v in lrs):
        raise ValueError(f"learning_rates: values in (0, 1], not {lrs!r}")
    if not all(v >= 0.0 and math.isfinite(v) for v in lams):
        raise ValueError(f"lambdas: finite values >= 0, not {lams!r}")
    if min_child_weight == 0 and not all(v > 0.0 for v in lams):
        raise ValueError("min_child_weight = 0 needs every lambda > 0: a leaf could divide by zero")
    F = folds if folds > 1 else 0
    if (F + 1) * len(lrs) * len(lams) > BOOST_MAX_MODELS:
        raise ValueError(f"(folds + 1) x {len(lrs)} learning rates x {len(lams)} lambdas = {(F + 1) * len(lrs) * len(lams)} "
                         f"models: at most {BOOST_MAX_MODELS} per call")
    if folds == 1 and len(lrs) * len(lams) != 1:
        raise ValueError("folds=1 is a plain fit without CV: it takes exactly one learning rate and one lambda")
    if not isinstance(X, torch.Tensor) or X.dim() != 2:
        raise ValueError(f"X: a 2-D tensor, not {getattr(X, 'shape', type(X))}")
    n, d = X.shape
    if X.dtype != torch.float32:
        raise ValueError(f"X: an fp32 tensor, not {X.dtype}")
    if not 1 <= d <= BOOST_MAX_D:
        raise ValueError(f"X: d = {d} outside 1..{BOOST_MAX_D}")
    if not isinstance(y, torch.Tensor) or y.dim() != 1 or y.shape[0] != n:
        raise ValueError(f"y: a 1-D tensor [{n}] -- one target, binary labels")
    if objective == "squared":
        if y.dtype != torch.float32:
            raise ValueError(f'y: an fp32 tensor for objective="squared", not {y.dtype}')
    else:
        if y.dtype.is_floating_point or y.dtype.is_complex or y.dtype == torch.bool:
            raise ValueError(f'y: an int tensor of labels in {{0, 1}} (-1 = unlabelled) for objective="logistic", not {y.dtype}')
        if n and (int(y.min()) < -1 or int(y.max()) > 1):
            raise GaeHipError(f"boost: labels in {{0, 1}} (-1 = unlabelled), got {int(y.min())}..{int(y.max())}")
    return lrs, lams, F


def _keep(rows, n, dev):
    """bool [n] on the device: the rows ``rows`` (ids or a mask; None: all) names"""
    if rows is None:
        return torch.ones(n, dtype=torch.bool, device=dev)
    if not isinstance(rows, torch.Tensor) or rows.dim() != 1 or rows.dtype.is_floating_point or rows.dtype.is_complex:
        raise ValueError(f"rows: a 1-D int tensor of row ids or a bool mask [{n}]")
    rows = rows.to(dev)
    if rows.dtype == torch.bool:
        if rows.shape[0] != n:
            raise ValueError(f"rows: a bool mask of {rows.shape[0]} entries for {n} rows")
        return rows.clone()
    if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= n):
        raise ValueError(f"rows: row ids outside 0..{n - 1}")
    keep = torch.zeros(n, dtype=torch.bool, device=dev)
    keep[rows.long()] = True
    return keep


def _gain_importances(feature, gain, d):
    on = feature >= 0
    f, w = feature[on], gain[on]
    sums = [math.fsum(w[f == q].tolist()) for q in range(d)]
    total = math.fsum(sums)
    return torch.tensor([s / total if total > 0.0 else 0.0 for s in sums], dtype=torch.float64)


def _choose(curve, ok):
    """(cfg, round index) of the smallest value of ``curve`` (a list of rows) among the eligible configurations, ties to the
    lower cfg, then the lower round; (-1, -1): none"""
    best, at = None, (-1, -1)
    for c, row in enumerate(curve):
        if not ok[c]:
            continue
        for r, v in enumerate(row):
            if not math.isnan(v) and (best is None or v < best):      # a strict <: ties keep the earlier point
                best, at = v, (c, r)
    return at


def boost(X, y, objective="squared", n_rounds=100, *, max_depth=4, learning_rates=(0.1,), lambdas=(1.0,),
          min_child_weight=1.0, min_samples_leaf=1, min_gain=0.0, max_features=1.0, max_bins=64, folds=5, fold=None,
          rows=None, seed=0, check_every=16, oof=False):
    """``BoostResult`` of gradient-boosted histogram trees on the rows of ``X`` [n, d] (fp32, on the GPU; read in place when
    the inner stride is 1).  ``objective="squared"``: ``y`` fp32 [n], the loss (F - y)^2 / 2; ``"logistic"``: ``y`` an int
    tensor [n] in {0, 1} (-1: unlabelled, the row is never read), the log-loss of sigma(F).  Each round fits one tree of
    depth <= ``max_depth`` to the gradients g and Hessians h of the running score F: a split maximises G_L^2 / (H_L +
    lambda) + G_R^2 / (H_R + lambda), needs ``min_samples_leaf`` rows and ``min_child_weight`` of H on both sides and a gain
    above ``min_gain``; a leaf adds -lr G / (H + lambda).  ``max_features`` (an int or a float share) features are drawn per
    node.  A configuration is one pair of ``learning_rates x lambdas``; (folds + 1) x n_cfg models -- per configuration one
    per fold and one on all rows -- train side by side, each fold model scoring its held-out rows after every round.  The
    result is the all-rows model of the pair and the round count with the smallest pooled held-out loss among the
    configurations whose models all stayed finite (ties: the lower configuration, then the fewer rounds).  ``rows``: an int
    tensor of row ids or a bool mask [n]; ``fold``: an int tensor [n] in -1..folds-1 (-1: left out, a test set), default a
    permutation seeded by ``seed`` dealt round-robin; rows outside ``rows``, with ``fold = -1`` or ``y = -1`` are never
    read.  ``folds=1``: a plain fit of one configuration.  ``check_every``: rounds between two reads of the 32-byte status
    block; no result depends on it.  ``oof=True`` also fits the chosen configuration's models once more for best_round
    rounds and returns every row's held-out score (``oof_score``).

    Results have the same bits run to run, for any row stride, stream or ``check_every``, and for a configuration fitted
    alone or inside a grid.  d <= 256, max_bins <= 256, max_depth 1..8, n_rounds <= 4096, <= 256 models, learning rates in
    (0, 1], lambdas >= 0, ``min_child_weight > 0`` or every lambda > 0.  A non-finite value in a listed row, or no
    configuration that stayed finite, raises GaeHipError; there is no CPU fallback."""
    lrs, lams, F = _options(X, y, objective, n_rounds, max_depth, learning_rates, lambdas, min_child_weight, min_samples_leaf,
                            min_gain, max_features, max_bins, folds, seed, check_every)
    if fold is not None:
        _fold_arg(fold, X.shape[0], folds)
    cfgs = [(lr, lam) for lr in lrs for lam in lams]
    n_cfg, Mo, R = len(cfgs), (F + 1) * len(cfgs), n_rounds
    with torch.no_grad():
        X, ldx, n, d = _rows(X, "boost")
        dev = X.device
        y = _gpu(y, "boost: y").detach()
        if y.device != dev:
            raise GaeHipError(f"boost: y must be on {dev}, not on {y.device}")
        m_feat = max_features if _whole(max_features) else max(1, int(max_features * d))
        if not 1 <= m_feat <= d:
            raise ValueError(f"max_features = {max_features!r}: 1..{d} features")
        with _on_device(dev):
            keep = _keep(rows, n, dev)
            fold_all = (_default_fold(n, max(F, 1), seed) if fold is None else fold.long()).to(dev)
            keep &= fold_all >= 0
            if objective == "logistic":
                keep &= y >= 0
            listed = keep.nonzero().reshape(-1).to(torch.int32)            # ascending row ids
            n_used = int(listed.shape[0])
            if n_used < 1:
                raise GaeHipError("boost: no rows to train on")
            sel = listed.long()
            fo = fold_all.index_select(0, sel).to(torch.int32).contiguous()
            if F:
                sizes = torch.bincount(fo.long(), minlength=F).cpu()
                if int(sizes.min()) == 0:
                    raise ValueError(f"fold: fold {int(sizes.argmin())} holds no listed rows (sizes {sizes.tolist()})")
            nbytes = _ws_bytes("gae_boost_workspace_bytes", n_used, d, max_bins, max_depth, F, n_cfg)    # shape errors first
            ys = y.index_select(0, sel).float().contiguous()
            ys_h = ys.double().cpu()
            if objective == "squared":
                if not bool(torch.isfinite(ys_h).all()):
                    raise GaeHipError("boost: the listed rows of y hold non-finite values")
                base = float(torch.tensor(math.fsum(ys_h.tolist()) / n_used).float())
                spread = float((ys_h - base).abs().max())
                exponent = 0 if spread == 0.0 else 29 - math.frexp(spread)[1]
            else:
                base, exponent = 0.0, 30
            Xs = X.index_select(0, sel)
            edges, n_edges = _edges(Xs, max_bins)
            status = torch.zeros(STATUS_WORDS, dtype=torch.int64, device=dev)
            codes = torch.empty(n_used, d, dtype=torch.uint8, device=dev)
            _lib.call("gae_forest_bin", _ptr(X), ldx, n, d, _ptr(listed), n_used, _ptr(edges), _ptr(n_edges), max_bins,
                      _ptr(codes), _ptr(status), _stream())
            M = 2 ** (max_depth + 1) - 1
            ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)

            def fit(pairs, rounds):
                k = len(pairs)
                i32 = dict(dtype=torch.int32, device=dev)
                f64 = dict(dtype=torch.float64, device=dev)
                out = dict(feature=torch.empty(k, rounds, M, **i32), tbin=torch.empty(k, rounds, M, **i32),
                           threshold=torch.empty(k, rounds, M, dtype=torch.float32, device=dev),
                           left=torch.empty(k, rounds, M, **i32), count=torch.empty(k, rounds, M, **i32),
                           value=torch.empty(k, rounds, M, **f64), gain=torch.empty(k, rounds, M, **f64),
                           n_nodes=torch.empty(k, rounds, **i32), loss=torch.empty((F + 1) * k, rounds + 1, **f64),
                           correct=torch.empty((F + 1) * k, rounds + 1, dtype=torch.int64, device=dev),
                           score=torch.empty((F + 1) * k, n_used, **f64), bad=torch.empty((F + 1) * k, **i32))
                lr_c = (ctypes.c_double * k)(*[p[0] for p in pairs])
                lam_c = (ctypes.c_double * k)(*[p[1] for p in pairs])

                def launch():
                    _lib.call("gae_boost_fit", _ptr(codes), _ptr(n_edges), _ptr(edges), n_used, d, max_bins, _ptr(ys),
                              _ptr(fo) if F else None, F, OBJECTIVES[objective], base, exponent, lr_c, lam_c, k, rounds,
                              max_depth, m_feat, min_samples_leaf, float(min_child_weight), float(min_gain), seed, check_every,
                              _ptr(out["feature"]), _ptr(out["tbin"]), _ptr(out["threshold"]), _ptr(out["left"]),
                              _ptr(out["count"]), _ptr(out["value"]), _ptr(out["gain"]), _ptr(out["n_nodes"]),
                              _ptr(out["loss"]), _ptr(out["correct"]), _ptr(out["score"]), _ptr(out["bad"]), _ptr(status),
                              _ptr(ws), ws.numel(), _stream())
                _timed(("boost", n_used, d, k * (F + 1), rounds, max_depth, max_bins), launch)
                st = status.cpu()
                if int(st[0]):
                    raise GaeHipError(f"boost: {int(st[0])} values of the {n_used} listed rows of X are not finite")
                if int(st[1]):
                    raise GaeHipError(f"boost: the device reported error flags 0x{int(st[1]):x} (1 row ids, 2 node tables, "
                                      f"4 bin codes, 8 targets / labels, 16 fold ids)")
                return out

            out = fit(cfgs, R)
            bad = out["bad"].cpu().reshape(n_cfg, F + 1)
            info = (bad != 0).any(1).to(torch.int32)
            ok = (info == 0).tolist()
            nan = float("nan")
            cv_rmse = cv_r2 = cv_logloss = cv_acc = nan
            if F:
                loss = out["loss"].cpu().reshape(n_cfg, F + 1, R + 1)
                pooled = loss[:, 0, 1:].clone()
                for k in range(1, F):
                    pooled = pooled + loss[:, k, 1:]                           # folds ascending, plain fp64 additions
                cv_curve = pooled / float(n_used)
                bc, br = _choose(cv_curve.tolist(), ok)
                if bc < 0:
                    raise GaeHipError("boost: no configuration whose models all stayed finite")
                if objective == "logistic":
                    correct = out["correct"].cpu().reshape(n_cfg, F + 1, R + 1)
                    cv_logloss = float(cv_curve[bc, br])
                    cv_acc = sum(int(correct[bc, k, br + 1]) for k in range(F)) / float(n_used)
                else:
                    mean = math.fsum(ys_h.tolist()) / n_used
                    c = ys_h - mean
                    sst = math.fsum((c * c).tolist())
                    cv_rmse = math.sqrt(float(cv_curve[bc, br]))
                    cv_r2 = 1.0 - float(pooled[bc, br]) / sst if sst > 0.0 else nan
            else:
                cv_curve = torch.full((n_cfg, R), nan, dtype=torch.float64)
                bc, br = 0, R - 1
                if not ok[0]:
                    raise GaeHipError("boost: the model did not stay finite")
            best_round = br + 1
            imp = _gain_importances(out["feature"][bc, :best_round].cpu(), out["gain"][bc, :best_round].cpu(), d)
            oof_score = None
            if oof:
                if not F:
                    raise ValueError("oof=True needs folds >= 2")
                again = fit([cfgs[bc]], best_round)
                oof_score = again["score"][:F].gather(0, fo.long().reshape(1, -1)).reshape(-1)
    return BoostResult(out["feature"][bc], out["tbin"][bc], out["threshold"][bc], out["left"][bc], out["count"][bc],
                       out["value"][bc], out["gain"][bc], out["n_nodes"][bc], base, edges, n_edges, cfgs[bc][0], cfgs[bc][1],
                       best_round, bc, cv_curve.to(dev), cv_rmse, cv_r2, cv_logloss, cv_acc, imp.to(dev), info.to(dev),
                       out["score"][bc * (F + 1) + F], objective, n_used, oof_score)


def boost_predict(result, X, n_rounds=None, status=None):
    """fp64 [m]: every row of ``X`` [m, d] (fp32, on the model's GPU, any row stride) walks the first ``n_rounds`` trees of
    ``result`` (None: best_round) on the raw floats (left iff x[feature] <= threshold); the leaves' values are added to
    base_score in ascending round order.  A row holding a non-finite feature gets NaN and is counted in ``status`` (an
    int64 [4] device tensor the caller zeroed: word 0 counts such rows, word 1 holds error flags; None: not reported).  No
    host synchronisation."""
    with torch.no_grad():
        X, ldx, m, d = _rows(X, "boost_predict")
        dev = result.feature.device
        R, M = result.feature.shape
        r = result.best_round if n_rounds is None else n_rounds
        if not _whole(r) or not 0 <= r <= R:
            raise ValueError(f"n_rounds: an integer in 0..{R}, not {n_rounds!r}")
        if X.device != dev or d != result.edges.shape[0]:
            raise GaeHipError(f"boost_predict: X must be [m, {result.edges.shape[0]}] on {dev}, got {tuple(X.shape)} on "
                              f"{X.device}")
        status = _status_arg(status, STATUS_WORDS, dev, "boost_predict")
        out = torch.empty(m, dtype=torch.float64, device=dev)
        with _on_device(dev):
            _lib.call("gae_boost_predict", _ptr(X), ldx, m, d, r, M, _ptr(result.feature), _ptr(result.threshold),
                      _ptr(result.left), _ptr(result.value), float(result.base_score), _ptr(out), _ptr(status), _stream())
    return out
