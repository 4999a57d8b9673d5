"""Host-side checks the heads on a frozen feature share (ridge, logreg, mlp, forest, boost, pca, tsne, cluster, knn,
tanimoto): the row layout of ``X`` and ``y``, the lambda path, the fold lists, listed rows, a caller's status tensor, the
tree options, the bin edges, and the result type, limits, option checks and launch of the two row searches.  Every head
imports from here and from ``_base``; none imports from another head.  Each message names the caller through ``who``.

Part of the package gae_dgl_amd.ops."""
import collections
import math

import torch

from .. import _lib
from .._lib import GaeHipError
from ._base import _f32, _gpu, _on_device, _ptr, _stream, _timed, _ws_bytes

MAX_FOLDS = 32                                                     # ridge and logreg: gae_ridge_stats' limit
_CV_PATH = [10.0 ** (e / 2.0) for e in range(-6, 7)]               # 10^-3 .. 10^3, 13 values

KNNResult = collections.namedtuple("KNNResult", ["index", "value"])
KNNResult.__doc__ = """index int32 [m, k] (rows of the database, -1 = padding), value fp32 [m, k]: the squared distance
("l2", ascending), the inner product ("dot") or the cosine ("cosine"), both descending; padding holds +inf / -inf"""
KNN_MAX_K, KNN_MAX_SPLITS = 64, 16                                 # the row searches: gae_knn and gae_tanimoto_knn


def _rows(X, who):
    """(X, ldx, n, d): a 2-D fp32 device tensor as it is when its inner stride is 1 (a column slice of a wider
    buffer is read in place), else a contiguous copy"""
    X = _f32(_gpu(X, f"{who}: X"), f"{who}: X").detach()
    if X.dim() != 2:
        raise GaeHipError(f"{who}: X must be 2-D, got {tuple(X.shape)}")
    n, d = X.shape
    if d > 0 and (X.stride(1) != 1 or (n > 1 and X.stride(0) < d)):
        X = X.contiguous()
    return X, (X.stride(0) if n > 1 else max(d, 1)), n, d


def _targets(y, n, dev, who):
    """(Y fp32 [n, t] in ``_rows``' layout, ldy, t) of the targets ``y``: [n] or [n, t], any float dtype, on ``dev``"""
    y = _gpu(y, f"{who}: y").detach()
    if y.device != dev or y.dim() not in (1, 2) or y.shape[0] != n or not y.dtype.is_floating_point:
        raise GaeHipError(f"{who}: y must be a float tensor [{n}] or [{n}, t] on {dev}, got {tuple(y.shape)} "
                          f"{y.dtype} on {y.device}")
    Y, ldy, _, t = _rows(y.reshape(n, 1).float() if y.dim() == 1 else y.float(), who)
    return Y, ldy, t


def _status_arg(status, words, dev, who):
    """the caller's status tensor (int64 [words] on ``dev``, contiguous, zeroed by the caller), or a fresh one for None"""
    if status is None:
        return torch.zeros(words, dtype=torch.int64, device=dev)
    if not (isinstance(status, torch.Tensor) and status.dtype == torch.int64 and status.numel() == words
            and status.device == dev and status.is_contiguous()):
        raise GaeHipError(f"{who}: status must be a contiguous int64 [{words}] tensor on {dev}")
    return status


# ------------------------------------------------------------------ the row searches (knn, tanimoto_knn)
def _search_options(X, k, exclude_self, splits):
    """(same, k as an int, flags): ``same`` is a search of Q against itself (``X is None``), which leaves every row out of
    its own list unless ``exclude_self`` says otherwise"""
    if k is None or isinstance(k, bool) or int(k) != k:
        raise ValueError(f"k: an integer in 1..{KNN_MAX_K}, not {k!r}")
    if isinstance(splits, bool) or int(splits) != splits or not 0 <= splits <= KNN_MAX_SPLITS:
        raise ValueError(f"splits: 0 (auto) or 1..{KNN_MAX_SPLITS}, not {splits!r}")
    same = X is None
    if exclude_self is None:
        exclude_self = same
    if exclude_self and not same:
        raise ValueError("exclude_self needs X=None: rows of a separate X share no index with the queries")
    return same, int(k), (_lib.KNN_EXCLUDE_SAME_INDEX if exclude_self else 0)


def _search(entry, label, dev, sizes, args):
    """``KNNResult`` of the row search ``entry(*args, index, value, ldo, workspace, bytes, stream)`` on ``dev``, timed as
    ``label``; ``sizes`` = (m, n, width, k, splits) is what its workspace query takes"""
    m, kk = sizes[0], max(sizes[3], 1)
    index = torch.empty(m, kk, dtype=torch.int32, device=dev)
    value = torch.empty(m, kk, dtype=torch.float32, device=dev)
    with _on_device(dev):
        nbytes = _ws_bytes(entry + "_workspace_bytes", *sizes)
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)

        def launch():
            _lib.call(entry, *args, _ptr(index), _ptr(value), kk, _ptr(ws), ws.numel(), _stream())
        _timed(label, launch)
    return KNNResult(index, value)


# ------------------------------------------------------------------ the lambda path and the folds
def _lambda_path(lambdas, folds, max_lambdas, default, max_folds=MAX_FOLDS):
    """(lambdas as a list of floats, folds as an int): ``lambdas`` is None (``default``), a tensor, a scalar or an
    iterable"""
    if isinstance(folds, bool) or int(folds) != folds or not 1 <= folds <= max_folds:
        raise ValueError(f"folds: an integer in 1..{max_folds}, not {folds!r}")
    if lambdas is None:
        lambdas = list(default)
    elif isinstance(lambdas, torch.Tensor):
        lambdas = lambdas.detach().double().cpu().reshape(-1).tolist()
    else:
        lambdas = [float(v) for v in (lambdas if hasattr(lambdas, "__iter__") else [lambdas])]
    if not 1 <= len(lambdas) <= max_lambdas:
        raise ValueError(f"lambdas: 1..{max_lambdas} values, not {len(lambdas)}")
    if not all(v >= 0.0 and math.isfinite(v) for v in lambdas):
        raise ValueError(f"lambdas: finite values >= 0, not {lambdas!r}")
    if int(folds) == 1 and len(lambdas) != 1:
        raise ValueError(f"folds=1 is a plain fit without CV: it takes exactly one lambda, not {len(lambdas)}")
    return lambdas, int(folds)


def _default_fold(n, F, seed):
    """int64 [n] on the host: a permutation seeded by ``seed``, dealt round-robin to F folds"""
    if F == 1:
        return torch.zeros(n, dtype=torch.int64)
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    perm = torch.randperm(n, generator=g)
    fold = torch.empty(n, dtype=torch.int64)
    fold[perm] = torch.arange(n) % F                                   # a seeded permutation dealt round-robin
    return fold


def _fold_arg(fold, n, F):
    """a caller's ``fold``: an int tensor [n] with values in -1..F-1"""
    if not isinstance(fold, torch.Tensor) or fold.dtype.is_floating_point or fold.dtype == torch.bool \
            or fold.dim() != 1 or fold.shape[0] != n:
        raise ValueError(f"fold: an int tensor [{n}] with values in -1..{F - 1}")
    if n and (int(fold.min()) < -1 or int(fold.max()) >= F):
        raise ValueError(f"fold: values in -1..{F - 1} (-1 = left out), got {int(fold.min())}..{int(fold.max())}")


def _fold_lists(fold, n, F, seed, dev):
    """(rows int32 [n_used], fold_ptr int32 [F + 1], counts int64 [F] on the host): the rows stably sorted by fold, -1
    (left out) dropped"""
    if fold is None:
        fold = _default_fold(n, F, seed).to(dev)
    else:
        _fold_arg(fold, n, F)
        fold = fold.to(dev).long()
    counts = torch.bincount(fold + 1, minlength=F + 1)[1:].cpu()
    if int(counts.min()) == 0:
        raise ValueError(f"fold: fold {int(counts.argmin())} holds no rows (sizes {counts.tolist()})")
    key = torch.where(fold < 0, torch.full_like(fold, F), fold)
    order = torch.sort(key, stable=True).indices
    n_used = int(counts.sum())
    rows = order[:n_used].to(torch.int32).contiguous()
    fold_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)]).to(torch.int32).to(dev)
    return rows, fold_ptr, counts


def _choose(ok, score):
    """index of the smallest score among the eligible lambdas, the LOWER index among equal scores; -1: none"""
    best = -1
    for l, (good, v) in enumerate(zip(ok, score)):
        if good and not math.isnan(v) and (best < 0 or v < score[best]):
            best = l                                                   # a strict <: ties go to the lower index
    return best


def _listed(rows, n, dev, who):
    """int32 [n_used] row ids on the device, or None for all rows in order"""
    if rows is None:
        return None
    if not isinstance(rows, torch.Tensor) or rows.dim() != 1 or rows.dtype.is_floating_point or rows.dtype.is_complex:
        raise GaeHipError(f"{who}: rows must be a 1-D int tensor of row ids or a bool mask [{n}]")
    rows = _gpu(rows, f"{who}: rows")
    if rows.device != dev:
        raise GaeHipError(f"{who}: rows on {rows.device}, X on {dev}")
    if rows.dtype == torch.bool:
        if rows.shape[0] != n:
            raise GaeHipError(f"{who}: a bool mask of {rows.shape[0]} entries for {n} rows")
        return rows.nonzero().reshape(-1).to(torch.int32)
    if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= n):
        raise GaeHipError(f"{who}: row ids outside 0..{n - 1}")
    return rows.to(torch.int32).contiguous()


# ------------------------------------------------------------------ histogram trees (forest, boost)
def _whole(v):
    return not isinstance(v, bool) and isinstance(v, int)


def _check_max_bins(v, most):
    if not _whole(v) or not 2 <= v <= most:
        raise ValueError(f"max_bins: an integer in 2..{most}, not {v!r}")


def _check_min_samples_leaf(v):
    if not _whole(v) or not 1 <= v < 2 ** 30:
        raise ValueError(f"min_samples_leaf: an integer >= 1, not {v!r}")


def _check_max_features(v):
    if not (v >= 1 if _whole(v) else isinstance(v, float) and 0.0 < v <= 1.0):
        raise ValueError(f"max_features: an integer in 1..d or a float in (0, 1], not {v!r}")


def _check_seed(v):
    if not _whole(v) or not 0 <= v < 2 ** 64:
        raise ValueError(f"seed: an integer in 0..2^64 - 1, not {v!r}")


def _edges(Xs, max_bins):
    """(edges fp32 [d, max_bins - 1] padded with +inf, n_edges int32 [d]) of the listed rows ``Xs``: the rule of the K26
    header comment, from one column sort"""
    n, d = Xs.shape
    E = max_bins - 1
    dev = Xs.device
    S = Xs.sort(dim=0).values
    new = torch.zeros(n, d, dtype=torch.bool, device=dev)
    new[1:] = S[1:] != S[:-1]
    lossless = (new.sum(0) + 1) <= max_bins
    edges = torch.full((d, E), float("inf"), dtype=torch.float32, device=dev)

    def place(marks, values_at):
        at = marks.t().nonzero()                                       # (f, i) in ascending f, then i
        f, i = at[:, 0], at[:, 1]
        cnt = torch.bincount(f, minlength=d)
        rank = torch.arange(f.shape[0], device=dev) - (cnt.cumsum(0) - cnt)[f]
        edges[f, rank] = values_at(f, i)
        return cnt

    def midpoint(f, i):
        a, b = S[i - 1, f], S[i, f]
        mid = ((a.double() + b.double()) / 2).float()
        return torch.where(mid >= b, a, mid)                           # a <= edge < b
    cnt_a = place(new & lossless, midpoint)
    idx = (torch.arange(1, max_bins, device=dev, dtype=torch.int64) * n) // max_bins
    Q = S[idx]                                                         # [E, d]
    keep = torch.ones(E, d, dtype=torch.bool, device=dev)
    keep[1:] = Q[1:] != Q[:-1]
    cnt_b = place(keep & ~lossless, lambda f, k: Q[k, f])
    return edges + 0.0, torch.where(lossless, cnt_a, cnt_b).to(torch.int32)        # (an edge of -0 is stored as +0)
