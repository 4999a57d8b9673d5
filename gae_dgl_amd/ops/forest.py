"""A random forest regressor on a frozen feature (K26, gae_forest_bin / gae_forest_fit / gae_forest_predict): the "GAE +
Random Forest" row of the reference's chemistry table on the device.  Histogram trees grown level by level, all trees of
a call at once; every accumulated quantity is an integer (bin codes, fixed-point int64 targets, integer histogram cells),
so the integer atomics the kernels use are exact: no float atomics, the same bits run to run, for any row stride and
stream.  ``GAE.forest_graphs``; ``python -m gae_dgl_amd.embed --forest``.  Regression only; gradient boosting on the same
cells, with binary classification, is ``ops.boost`` (K30).

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import collections
import ctypes
import math

import torch

import gae_dgl_amd.ops as _ops
from .. import _lib
from .._lib import GaeHipError
from ._base import _on_device, _ptr, _stream, _timed, _ws_bytes
from ._heads import (_check_max_bins, _check_max_features, _check_min_samples_leaf, _check_seed, _edges, _listed, _rows,
                     _status_arg, _targets, _whole)

__all__ = ['ForestResult', 'forest', 'forest_predict', 'FOREST_MAX_D', 'FOREST_MAX_T', 'FOREST_MAX_TREES',
           'FOREST_MAX_DEPTH', 'FOREST_MAX_BINS', 'FOREST_SPLIT_ROWS']

FOREST_MAX_D, FOREST_MAX_T, FOREST_MAX_TREES, FOREST_MAX_DEPTH, FOREST_MAX_BINS = 256, 8, 1024, 16, 256
FOREST_SPLIT_ROWS = _lib.FOREST_SPLIT_ROWS
STATUS_WORDS = 4          # gae_forest_status: int64 nonfinite, errors, reserved[2]


class ForestResult(collections.namedtuple("ForestResult", [
        "feature", "threshold_bin", "threshold", "left", "count", "value", "gain", "n_nodes", "edges", "n_edges",
        "oob_prediction", "oob_rmse", "oob_r2", "importances", "n_used", "pivot", "exponent"])):
    """The node tables [T, M] of T trees, M = min(2^(max_depth + 1) - 1, 2 n_boot - 1): feature int32 (-1 marks a leaf),
    threshold_bin int32, threshold fp32 (a row goes left iff x[feature] <= threshold), left int32 (the right child is
    left + 1), count int32, value fp64 [T, M, t] (the mean target of EVERY node), gain fp64; n_nodes int32 [T]; edges fp32
    [d, max_bins - 1] (+inf past n_edges int32 [d]); oob_prediction fp64 [n_used, t]: the mean over the trees that did
    not draw the row, NaN where every tree drew it; oob_rmse / oob_r2 fp64 [t] over the rows with at least one
    out-of-bag tree (exactly rounded sums on the host); importances fp64 [d]: sum of gain . count per feature,
    normalised to 1; n_used listed rows; pivot fp32 [t] and exponent (a list of t ints): the fixed-point frame of the
    targets.  With ``bootstrap=False`` there is no out-of-bag estimate: the oob_* fields hold NaN."""
    __slots__ = ()

    def predict(self, X, status=None):
        """fp64 [m, t]: the mean of the trees' leaf values for every row of ``X`` (``ops.forest_predict``)"""
        return _ops.forest_predict(self, X, status=status)


def _options(n_trees, max_depth, max_features, min_samples_leaf, max_bins, bootstrap, max_samples, seed):
    if not _whole(n_trees) or not 1 <= n_trees <= FOREST_MAX_TREES:
        raise ValueError(f"n_trees: an integer in 1..{FOREST_MAX_TREES}, not {n_trees!r}")
    if not _whole(max_depth) or not 1 <= max_depth <= FOREST_MAX_DEPTH:
        raise ValueError(f"max_depth: an integer in 1..{FOREST_MAX_DEPTH}, not {max_depth!r}")
    _check_max_bins(max_bins, FOREST_MAX_BINS)
    _check_min_samples_leaf(min_samples_leaf)
    if not isinstance(bootstrap, bool):
        raise ValueError(f"bootstrap: True or False, not {bootstrap!r}")
    _check_max_features(max_features)
    if max_samples is not None:
        if not bootstrap:
            raise ValueError("max_samples needs bootstrap=True: without the bootstrap every tree trains on every listed row")
        if _whole(max_samples):
            if max_samples < 1:
                raise ValueError(f"max_samples: an integer >= 1 or a float in (0, 1], not {max_samples!r}")
        elif not (isinstance(max_samples, float) and 0.0 < max_samples <= 1.0):
            raise ValueError(f"max_samples: an integer >= 1 or a float in (0, 1], not {max_samples!r}")
    _check_seed(seed)


def _fsum_scores(pred, y):
    """(rmse [t], r2 [t]) on the host over the rows whose prediction is not NaN, from exactly rounded sums"""
    t = y.shape[1]
    rmse, r2 = [], []
    for j in range(t):
        keep = ~torch.isnan(pred[:, j])
        p, v = pred[keep, j], y[keep, j]
        k = int(p.shape[0])
        if k == 0:
            rmse.append(float("nan")); r2.append(float("nan"))
            continue
        r = p - v
        sse = math.fsum((r * r).tolist())
        mean = math.fsum(v.tolist()) / k
        c = v - mean
        sst = math.fsum((c * c).tolist())
        rmse.append(math.sqrt(sse / k))
        r2.append(1.0 - sse / sst if sst > 0.0 else float("nan"))
    return rmse, r2


def _importances(feature, count, gain, d):
    """fp64 [d] on the host: per feature the exactly rounded sum of gain . count over the nodes that split on it"""
    on = feature >= 0
    f, w = feature[on], gain[on] * count[on].double()
    sums = [math.fsum(w[f == q].tolist()) for q in range(d)]
    total = math.fsum(sums)
    return torch.tensor([s / total if total > 0.0 else 0.0 for s in sums], dtype=torch.float64)


def forest(X, y, n_trees=100, *, max_depth=12, max_features=1.0, min_samples_leaf=1, max_bins=64, bootstrap=True,
           max_samples=None, rows=None, seed=0):
    """``ForestResult`` of a random forest regression of ``y`` ([n] or [n, t], 1 <= t <= 8, any float dtype, read as fp32)
    on the rows of ``X`` [n, d] (fp32, on the GPU; read in place when the inner stride is 1).  ``rows``: an int tensor of
    row ids or a bool mask [n] -- the training rows; rows outside it (a test set) are never read.  Every feature is cut
    into at most ``max_bins`` bins (lossless when a column has at most max_bins distinct values, evenly spaced order
    statistics otherwise); the targets become fixed point about their mean with a step of 2^-31 of their range, so every
    histogram cell is an integer and every tree is reproduced node for node by tests/forest_ref.py.  Each tree trains on a
    Philox bootstrap of ``max_samples`` rows (None: as many as listed; an int, or a float share of the listed rows) or,
    with ``bootstrap=False``, on every listed row; a split looks at ``max_features`` features (an int in 1..d or a float
    share, at least one) drawn per node.  Regression only (boosting and binary classification: ``ops.boost``).  1 <= d <= 256,
    n_trees <= 1024, max_depth <= 16, max_bins <= 256; a non-finite value in a listed row raises GaeHipError; there is no
    CPU fallback."""
    _options(n_trees, max_depth, max_features, min_samples_leaf, max_bins, bootstrap, max_samples, seed)
    with torch.no_grad():
        X, ldx, n, d = _rows(X, "forest")
        dev = X.device
        Y, ldy, t = _targets(y, n, dev, "forest")
        m_feat = max_features if isinstance(max_features, int) else max(1, int(max_features * d))
        if not 1 <= m_feat <= max(d, 1):
            raise ValueError(f"max_features = {max_features!r}: 1..{d} features")
        with _on_device(dev):
            lib = _lib.load()
            listed = _listed(rows, n, dev, "forest")
            n_used = n if listed is None else int(listed.shape[0])
            if n_used < 1:
                raise GaeHipError("forest: no rows to train on")
            if max_samples is None:
                n_boot = n_used
            else:
                n_boot = max_samples if isinstance(max_samples, int) else max(1, int(max_samples * n_used))
            # shape errors before any other work
            nbytes = _ws_bytes("gae_forest_workspace_bytes", n_used, d, t, n_trees, n_boot, max_depth, max_bins)
            Xs = X if listed is None else X.index_select(0, listed.long())
            Ys = Y if listed is None else Y.index_select(0, listed.long())
            edges, n_edges = _edges(Xs, max_bins)
            status = torch.zeros(STATUS_WORDS, dtype=torch.int64, device=dev)
            codes = torch.empty(n_used, d, dtype=torch.uint8, device=dev)
            _lib.call("gae_forest_bin", _ptr(X), ldx, n, d, _ptr(listed), n_used, _ptr(edges), _ptr(n_edges), max_bins,
                      _ptr(codes), _ptr(status), _stream())
            pivot = (Ys.double().sum(0) / n_used).float()                  # (a sum and ONE division, as the header states)
            spread = (Ys.double() - pivot.double()).abs().amax(0)
            host = torch.cat([status.double(), pivot.double(), spread]).cpu()          # the first read
            if int(host[1]):
                raise GaeHipError(f"forest: the device reported error flags 0x{int(host[1]):x} (row ids)")
            if int(host[0]):
                raise GaeHipError(f"forest: {int(host[0])} values of the {n_used} listed rows of X are not finite")
            piv_h, spread_h = host[STATUS_WORDS:STATUS_WORDS + t].tolist(), host[STATUS_WORDS + t:].tolist()
            if not all(math.isfinite(v) for v in piv_h + spread_h):
                raise GaeHipError(f"forest: the listed rows of y hold non-finite values")
            exponent = [0 if s == 0.0 else 30 - math.frexp(s)[1] for s in spread_h]
            M = min(2 ** (max_depth + 1) - 1, 2 * n_boot - 1)
            feature = torch.empty(n_trees, M, dtype=torch.int32, device=dev)
            tbin, left, count = torch.empty_like(feature), torch.empty_like(feature), torch.empty_like(feature)
            threshold = torch.empty(n_trees, M, dtype=torch.float32, device=dev)
            value = torch.empty(n_trees, M, t, dtype=torch.float64, device=dev)
            gain = torch.empty(n_trees, M, dtype=torch.float64, device=dev)
            n_nodes = torch.empty(n_trees, dtype=torch.int32, device=dev)
            inbag = torch.empty(n_trees, n_used, dtype=torch.uint8, device=dev) if bootstrap else None
            oob = torch.full((n_used, t), float("nan"), dtype=torch.float64, device=dev)
            ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
            piv_c = (ctypes.c_float * t)(*piv_h)
            exp_c = (ctypes.c_int32 * t)(*exponent)
            flags = _lib.FOREST_BOOTSTRAP if bootstrap else 0

            def launch():
                _lib.call("gae_forest_fit", _ptr(codes), _ptr(n_edges), _ptr(edges), n_used, d, max_bins, _ptr(Y), ldy, n, t,
                          _ptr(listed), piv_c, exp_c, n_trees, n_boot, max_depth, m_feat, min_samples_leaf, flags, seed,
                          _ptr(feature), _ptr(tbin), _ptr(threshold), _ptr(left), _ptr(count), _ptr(value), _ptr(gain),
                          _ptr(n_nodes), M, _ptr(inbag), _ptr(status), _ptr(ws), ws.numel(), _stream())
                if bootstrap:
                    _lib.call("gae_forest_predict", _ptr(Xs), Xs.stride(0) if n_used > 1 else d, n_used, d, t, n_trees, M,
                              _ptr(feature), _ptr(threshold), _ptr(left), _ptr(value), _ptr(inbag), _ptr(oob),
                              _ptr(status), _stream())
            _timed(("forest", n_used, d, t, n_trees, max_depth, max_bins), launch)
            st = status.cpu()
            if int(st[1]) or int(st[0]):
                raise GaeHipError(f"forest: the device reported error flags 0x{int(st[1]):x} and {int(st[0])} non-finite "
                                  f"values in the listed rows")
            top = int(n_nodes.max())
            imp = _importances(feature[:, :top].cpu(), count[:, :top].cpu(), gain[:, :top].cpu(), d)
            if bootstrap:
                rmse, r2 = _fsum_scores(oob.cpu(), Ys.double().cpu())
            else:
                rmse = r2 = [float("nan")] * t
            f64 = dict(dtype=torch.float64, device=dev)
    return ForestResult(feature, tbin, threshold, left, count, value, gain, n_nodes, edges, n_edges, oob,
                        torch.tensor(rmse, **f64), torch.tensor(r2, **f64), imp.to(dev), n_used, pivot, exponent)


def forest_predict(result, X, status=None):
    """fp64 [m, t]: every row of ``X`` [m, d] (fp32, on the forest's GPU, any row stride) walks every tree of ``result`` on
    the raw floats (left iff x[feature] <= threshold) and gets the mean of the reached nodes' values.  A row holding a
    non-finite feature gets NaN and is counted in ``status`` (an int64 [4] device tensor the caller zeroed: word 0 counts
    such rows, word 1 holds error flags; None: not reported).  No host synchronisation."""
    with torch.no_grad():
        X, ldx, m, d = _rows(X, "forest_predict")
        dev = result.feature.device
        T, M = result.feature.shape
        t = result.value.shape[2]
        if X.device != dev or d != result.edges.shape[0]:
            raise GaeHipError(f"forest_predict: X must be [m, {result.edges.shape[0]}] on {dev}, got {tuple(X.shape)} on "
                              f"{X.device}")
        status = _status_arg(status, STATUS_WORDS, dev, "forest_predict")
        out = torch.empty(m, t, dtype=torch.float64, device=dev)
        with _on_device(dev):
            _lib.call("gae_forest_predict", _ptr(X), ldx, m, d, t, T, M, _ptr(result.feature), _ptr(result.threshold),
                      _ptr(result.left), _ptr(result.value), None, _ptr(out), _ptr(status), _stream())
    return out
