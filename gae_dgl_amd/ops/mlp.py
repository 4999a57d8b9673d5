"""An MLP regression head on a frozen feature with a k-fold CV grid (K27, gae_mlp_fit / gae_mlp_predict): the "GAE + MLP"
row of the reference's chemistry table on the device.  One block per model, every fold model and the all-rows model of
every (lr, alpha) configuration in one grid; every matrix product element is one fp32 fma chain on the fp32-input matrix
instruction, so a fit has the same bits run to run and for any cut into launches (tests/mlp_ref.py restates it).
``GAE.mlp_graphs``; ``python -m gae_dgl_amd.embed --mlp``.  Regression only, ReLU only; no early stopping.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import collections
import math

import torch

import gae_dgl_amd.ops as _ops
from .. import _lib
from .._lib import GaeHipError
from ._base import _on_device, _ptr, _stream, _timed, _ws_bytes
from ._heads import _check_seed, _choose, _fold_lists, _rows, _status_arg, _targets, _whole

__all__ = ['MLPResult', 'mlp', 'mlp_predict', 'mlp_usable', 'mlp_load_head', 'MLP_MAX_WIDTH', 'MLP_MAX_T', 'MLP_MAX_MODELS', 'MLP_MAX_FOLDS',
           'MLP_LAUNCH_ROW_VISITS']

MLP_MAX_WIDTH, MLP_MAX_T, MLP_MAX_MODELS, MLP_MAX_FOLDS = 128, 8, 4096, 32
MLP_LAUNCH_ROW_VISITS = _lib.MLP_LAUNCH_ROW_VISITS
STATUS_WORDS = 4          # gae_mlp_status: int64 nonfinite_rows, errors, reserved[2]
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


class MLPResult(collections.namedtuple("MLPResult", [
        "weights", "biases", "lr", "alpha", "lrs", "alphas", "cv_rmse", "cv_r2", "cv_sse", "loss_curve", "info", "n_used",
        "fold_counts", "shift", "scale", "hidden", "state"])):
    """weights / biases: per layer fp32 [ensemble, out, in] / [ensemble, out] (``torch.nn.Linear`` layout) of the models
    fitted on all listed rows at the chosen (``lr``, ``alpha``); they act on the scaled values (v - shift) * scale (shift,
    scale fp32 [d + t]: features, then targets).  lrs / alphas: the configurations, index c = i_lr * len(alphas) + i_alpha;
    cv_rmse / cv_r2 fp64 [C, t] from the SSE pooled over the folds and averaged over the members (R2 against the SST of
    the listed rows about their overall mean); cv_sse fp64 [C, F, ensemble, t]; loss_curve fp64 [C, F + 1, ensemble,
    epochs] (index F: the all-rows model) and info int32 [C, F + 1, ensemble] as gae_mlp_fit reports them; n_used listed
    rows; fold_counts int64 [F]; hidden: the widths; state: the chosen models' state blocks.  With ``folds=1`` there is no
    CV: the cv_* tables hold NaN and the tables have one fold slot."""
    __slots__ = ()

    def predict(self, X, status=None):
        """fp64 [n, t]: the mean of the members' predictions, added in member order (``ops.mlp_predict``)"""
        return _ops.mlp_predict(self, X, status=status)

    def to_torch(self, member=0):
        """an ``nn.Sequential`` (Linear, ReLU, ..., Linear) of member ``member`` that takes RAW features and returns raw
        targets: the scaling is folded into the first and the last layer (in fp64, stored as fp32)"""
        return _sequential([w[member].double().cpu() for w in self.weights], [b[member].double().cpu() for b in self.biases],
                           self.shift.double().cpu(), self.scale.double().cpu())


def _sequential(Ws, bs, shift, scale):
    """Linear, ReLU, ..., Linear from fp64 host tensors, the scaling folded into the first and the last layer"""
    d = Ws[0].shape[1]
    Ws, bs = list(Ws), list(bs)
    W0 = Ws[0] * scale[None, :d]
    bs[0] = bs[0] - W0 @ shift[:d]
    Ws[0] = W0
    Ws[-1] = Ws[-1] / scale[d:, None]
    bs[-1] = bs[-1] / scale[d:] + shift[d:]
    layers = []
    for l, (W, b) in enumerate(zip(Ws, bs)):
        lin = torch.nn.Linear(W.shape[1], W.shape[0])
        with torch.no_grad():
            lin.weight.copy_(W.float()); lin.bias.copy_(b.float())
        layers.append(lin)
        if l < len(Ws) - 1:
            layers.append(torch.nn.ReLU())
    return torch.nn.Sequential(*layers)


def mlp_load_head(path, member=0):
    """the ``nn.Sequential`` of ``MLPResult.to_torch(member)`` from the .npz that ``embed --mlp_out`` wrote"""
    import numpy as np
    with np.load(path) as z:
        n_layers = len(z["hidden"]) + 1
        Ws = [torch.from_numpy(z[f"weight{l}"][member]).double() for l in range(n_layers)]
        bs = [torch.from_numpy(z[f"bias{l}"][member]).double() for l in range(n_layers)]
        return _sequential(Ws, bs, torch.from_numpy(z["shift"]).double(), torch.from_numpy(z["scale"]).double())


def _hidden(hidden):
    if isinstance(hidden, int) and not isinstance(hidden, bool):
        hidden = (hidden,)
    try:
        hidden = tuple(hidden)
    except TypeError:
        raise ValueError(f"hidden: one or two widths in 1..{MLP_MAX_WIDTH}, not {hidden!r}") from None
    if not 1 <= len(hidden) <= 2 or not all(isinstance(h, int) and not isinstance(h, bool) and 1 <= h <= MLP_MAX_WIDTH
                                            for h in hidden):
        raise ValueError(f"hidden: one or two widths in 1..{MLP_MAX_WIDTH}, not {hidden!r}")
    return hidden


def mlp_usable(d, hidden, t):
    """does K27 take the head ``d -> hidden -> t``?  Mirrors gae_mlp_workspace_bytes: False outside the limits (1 <= d,
    width <= 128, one or two hidden layers, 1 <= t <= 8) and where the weights and a row panel do not fit a block's LDS
    (128 -> 128 -> 128).  Asks the library; no launch, no GPU."""
    try:
        hidden = _hidden(hidden)
    except ValueError:
        return False
    return int(_lib.load().gae_mlp_workspace_bytes(int(d), hidden[0], hidden[1] if len(hidden) > 1 else 0, int(t), 1)) > 0


def _options(hidden, lrs, alphas, epochs, batch_size, folds, ensemble, seed, solver, momentum, shuffle, standardize):
    def values(v, name, low_ok):
        if isinstance(v, torch.Tensor):
            v = v.detach().double().cpu().reshape(-1).tolist()
        v = [float(x) for x in (v if hasattr(v, "__iter__") else [v])]
        if not v or not all(math.isfinite(x) and (x >= 0.0 if low_ok else x > 0.0) for x in v):
            raise ValueError(f"{name}: one or more finite values {'>= 0' if low_ok else '> 0'}, not {v!r}")
        return v
    hidden = _hidden(hidden)
    lrs, alphas = values(lrs, "lrs", False), values(alphas, "alphas", True)
    if not _whole(epochs) or not 1 <= epochs < 2 ** 31:
        raise ValueError(f"epochs: an integer >= 1, not {epochs!r}")
    if not _whole(batch_size) or not 1 <= batch_size < 2 ** 31:
        raise ValueError(f"batch_size: an integer >= 1, not {batch_size!r}")
    if not _whole(folds) or not 1 <= folds <= MLP_MAX_FOLDS:
        raise ValueError(f"folds: an integer in 1..{MLP_MAX_FOLDS}, not {folds!r}")
    if not _whole(ensemble) or ensemble < 1:
        raise ValueError(f"ensemble: an integer >= 1, not {ensemble!r}")
    C = len(lrs) * len(alphas)
    if folds == 1 and C != 1:
        raise ValueError(f"folds=1 is a plain fit without CV: it takes exactly one configuration, not {C}")
    M = (folds + 1 if folds > 1 else 1) * C * ensemble
    if M > MLP_MAX_MODELS:
        raise ValueError(f"(folds + 1) * configurations * ensemble = {M} models, at most {MLP_MAX_MODELS} per call")
    _check_seed(seed)
    if solver not in ("adam", "sgd"):
        raise ValueError(f"solver: 'adam' or 'sgd', not {solver!r}")
    if isinstance(momentum, bool) or not isinstance(momentum, (int, float)) or not 0.0 <= momentum < 1.0:
        raise ValueError(f"momentum: a value in [0, 1), not {momentum!r}")
    if momentum and solver != "sgd":
        raise ValueError("momentum belongs to solver='sgd'")
    if not isinstance(shuffle, bool) or not isinstance(standardize, bool):
        raise ValueError(f"shuffle, standardize: True or False, not {shuffle!r}, {standardize!r}")
    return hidden, lrs, alphas


def _mix(x):
    """splitmix64's finaliser"""
    x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return x ^ (x >> 31)


def model_seed(seed, config, fold, member):
    """the 64-bit seed of one model: a function of (seed, config, fold, member) alone; the all-rows model has fold = folds"""
    x = _mix(seed)
    for v in (config, fold, member):
        x = _mix(x ^ ((v + 1) * 0xD6E8FEB86659FD93 & 0xFFFFFFFFFFFFFFFF))
    return x


def _params(state, d, hidden, t):
    """per layer views (W [M, out, in], b [M, out]) into state blocks fp32 [M, S]"""
    widths = [d] + list(hidden) + [t]
    Ws, bs, o = [], [], _lib.MLP_STATE_HEADER
    for l in range(len(widths) - 1):
        out, inn = widths[l + 1], widths[l]
        Ws.append(state[:, o:o + out * inn].reshape(-1, out, inn)); o += out * inn
        bs.append(state[:, o:o + out]); o += out
    return Ws, bs


def mlp(X, y, hidden=(100,), *, lrs=(1e-3,), alphas=(1e-4,), epochs=200, batch_size=200, folds=5, fold=None, ensemble=1,
        seed=0, solver="adam", momentum=0.0, shuffle=True, standardize=True):
    """``MLPResult`` of an MLP regression ``d -> hidden -> t`` (ReLU, squared error, L2 penalty ``alpha``, Adam with
    beta = (0.9, 0.999), eps 1e-8, or plain SGD with ``momentum``) of ``y`` ([n] or [n, t], 1 <= t <= 8, any float dtype,
    read as fp32) on the rows of ``X`` [n, d] (fp32, on the GPU; read in place when the inner stride is 1).  The
    configurations are the pairs ``lrs x alphas``; one call trains ``(folds + 1) * C * ensemble`` models side by side --
    every fold model and the all-rows model of every configuration, ``ensemble`` members each, every model with its own
    seed derived from (seed, configuration, fold, member) -- and picks the configuration with the smallest mean over the
    targets of the pooled ``1 - cv_r2`` among those whose every model stayed finite (``info == 0``), ties to the lower
    index.  ``fold``: as in ``ops.ridge`` (-1: the row is left out and never read); ``folds=1``: no CV, exactly one
    configuration.  ``standardize``: train on (v - mean) / std of the listed rows, features and targets (fp32 mean and
    1 / std by torch; a zero spread gives scale 1); predictions come back in the targets' own units.  A fit is cut into
    launches of at most MLP_LAUNCH_ROW_VISITS row visits per model, with the same bits for any cut; the host reads the
    status once per launch and the tables once.  1 <= d, widths <= 128, one or two hidden layers, at most 4096 models; a
    non-finite value in a listed row, or no configuration whose models all stayed finite, raises GaeHipError; there is no
    CPU fallback."""
    hidden, lrs, alphas = _options(hidden, lrs, alphas, epochs, batch_size, folds, ensemble, seed, solver, momentum,
                                   shuffle, standardize)
    F, E, C = folds, ensemble, len(lrs) * len(alphas)
    with torch.no_grad():
        X, ldx, n, d = _rows(X, "mlp")
        dev = X.device
        Y, ldy, t = _targets(y, n, dev, "mlp")
        slots = F + 1 if F > 1 else 1                                  # models per (configuration, member)
        M = slots * C * E
        h1, h2 = hidden[0], hidden[1] if len(hidden) > 1 else 0
        with _on_device(dev):
            nbytes = _ws_bytes("gae_mlp_workspace_bytes", d, h1, h2, t, M)         # shape errors before any other work
            rows, fold_ptr, counts = _fold_lists(fold, n, F, seed, dev)
            n_used = int(rows.shape[0])
            ptr = fold_ptr.cpu().tolist()
            # the lists: per fold its training rows (every other fold, in the order of `rows`) and its own rows; then all
            pieces, lens = [], []
            if F > 1:
                for f in range(F):
                    pieces += [rows[:ptr[f]], rows[ptr[f + 1]:], rows[ptr[f]:ptr[f + 1]]]
                    lens += [n_used - (ptr[f + 1] - ptr[f]), ptr[f + 1] - ptr[f]]
            pieces.append(rows); lens.append(n_used)
            all_rows = torch.cat(pieces).contiguous()
            list_ptr = torch.tensor([0] + list(_accumulate(lens)), dtype=torch.int32, device=dev)
            n_lists = len(lens)
            train_l, eval_l, lr_l, al_l, seed_l = [], [], [], [], []
            for c in range(C):
                for f in range(slots):
                    for k in range(E):
                        last = f == slots - 1
                        train_l.append(n_lists - 1 if last else 2 * f)
                        eval_l.append(-1 if last else 2 * f + 1)
                        lr_l.append(lrs[c // len(alphas)]); al_l.append(alphas[c % len(alphas)])
                        seed_l.append(model_seed(seed, c, F if last else f, k))
            i32 = dict(dtype=torch.int32, device=dev)
            train_d, eval_d = torch.tensor(train_l, **i32), torch.tensor(eval_l, **i32)
            lr_d = torch.tensor(lr_l, dtype=torch.float32, device=dev)
            al_d = torch.tensor(al_l, dtype=torch.float32, device=dev)
            seed_d = torch.tensor([s - (1 << 64) if s >= 1 << 63 else s for s in seed_l], dtype=torch.int64, device=dev)
            sel = rows.long()
            everything = n_used == n
            Xs = X if everything else X.index_select(0, sel)
            Ys = Y if everything else Y.index_select(0, sel)
            if standardize:
                V = torch.cat([Xs, Ys], dim=1)
                shift = V.mean(0)
                std = V.std(0, unbiased=False)
                scale = torch.where(std > 0, 1.0 / std, torch.ones_like(std))
                shift, scale = shift.contiguous(), scale.contiguous()
            else:
                shift = torch.zeros(d + t, dtype=torch.float32, device=dev)
                scale = torch.ones(d + t, dtype=torch.float32, device=dev)
            status = torch.zeros(STATUS_WORDS, dtype=torch.int64, device=dev)
            loss_curve = torch.empty(M, epochs, dtype=torch.float64, device=dev)
            eval_sse = torch.empty(M, t, dtype=torch.float64, device=dev)
            info = torch.empty(M, dtype=torch.int32, device=dev)
            ws = torch.empty(int(nbytes) // 4, dtype=torch.float32, device=dev)
            per_launch = max(1, MLP_LAUNCH_ROW_VISITS // n_used)
            flags0 = _lib.MLP_SHUFFLE if shuffle else 0
            code = _lib.MLP_ADAM if solver == "adam" else _lib.MLP_SGD

            def launch(e0, e1):
                flags = flags0 | (_lib.MLP_FINAL if e1 == epochs else 0)
                _lib.call("gae_mlp_fit", _ptr(X), ldx, _ptr(Y), ldy, n, d, h1, h2, t, _ptr(shift), _ptr(scale),
                          _ptr(all_rows), all_rows.numel(), _ptr(list_ptr), n_lists, _ptr(train_d), _ptr(eval_d), _ptr(lr_d),
                          _ptr(al_d), _ptr(seed_d), M, batch_size, BETA1, BETA2, EPS, code, float(momentum), flags, e0, e1,
                          epochs, _ptr(loss_curve), _ptr(eval_sse), _ptr(info), _ptr(status), _ptr(ws), ws.numel() * 4,
                          _stream())
            for e0 in range(0, epochs, per_launch):
                e1 = min(epochs, e0 + per_launch)
                _timed(("mlp", n_used, d, hidden, t, M, e1 - e0), lambda: launch(e0, e1))
                st = status.cpu()                                      # the launch cut's one read
                if int(st[1]):
                    raise GaeHipError(f"mlp: the device reported error flags 0x{int(st[1]):x} (row lists)")
                if int(st[0]):
                    raise GaeHipError(f"mlp: {int(st[0])} entries of the row lists name rows that hold non-finite values")
            sst = ((Ys.double() - Ys.double().mean(0)) ** 2).sum(0)
            host = torch.cat([info.double(), eval_sse.reshape(-1), sst]).cpu()                     # the tables' one read
        info_h = host[:M].reshape(C, slots, E)
        sse_h = host[M:M + M * t].reshape(C, slots, E, t)
        sst_h = host[-t:]
        if F > 1:
            cv_sse = sse_h[:, :F]
            pooled = cv_sse.sum(1).mean(1)                             # [C, t]: folds added, members averaged
            cv_rmse = torch.sqrt(pooled / n_used)
            cv_r2 = 1.0 - pooled / sst_h
            ok = [bool((info_h[c] == 0).all()) for c in range(C)]
            score = [float((1.0 - cv_r2[c]).mean()) for c in range(C)]
        else:
            cv_sse = torch.full((C, 1, E, t), float("nan"), dtype=torch.float64)
            cv_rmse = cv_r2 = torch.full((C, t), float("nan"), dtype=torch.float64)
            ok, score = [bool((info_h[0] == 0).all())], [0.0]
        best = _choose(ok, score)
        if best < 0:
            raise GaeHipError(f"mlp: none of the {C} configurations kept every model finite "
                              f"(info = {info_h.int().tolist()})")
        S = ws.numel() // M
        blocks = ws.reshape(M, S)
        first = (best * slots + slots - 1) * E
        chosen = blocks[first:first + E].clone()
        Ws, bs = _params(chosen, d, hidden, t)
    return MLPResult(Ws, bs, lrs[best // len(alphas)], alphas[best % len(alphas)], lrs, alphas, cv_rmse.to(dev), cv_r2.to(dev),
                     cv_sse.to(dev), loss_curve.reshape(C, slots, E, epochs), info.reshape(C, slots, E), n_used, counts, shift,
                     scale, hidden, chosen)


def _accumulate(values):
    total = 0
    for v in values:
        total += v
        yield total


def mlp_predict(result, X, status=None):
    """fp64 [n, t]: for every row of ``X`` [n, d] (fp32, on the result's GPU, any row stride) the mean over the members of
    ``result`` of the model's prediction in the targets' own units, added in member order; each member's forward runs
    the chains of training (gae_mlp_predict).  A row holding a non-finite feature gets NaN and is counted in ``status``
    (an int64 [4] device tensor the caller zeroed; None: not reported).  No host synchronisation."""
    with torch.no_grad():
        X, ldx, n, d = _rows(X, "mlp_predict")
        dev = result.state.device
        E = result.state.shape[0]
        d0, t = result.weights[0].shape[2], result.weights[-1].shape[1]
        if X.device != dev or d != d0:
            raise GaeHipError(f"mlp_predict: X must be [n, {d0}] on {dev}, got {tuple(X.shape)} on {X.device}")
        if status is not None:                                         # (None: the kernel does not report)
            _status_arg(status, STATUS_WORDS, dev, "mlp_predict")
        hidden = result.hidden
        out = torch.empty(E, n, t, dtype=torch.float32, device=dev)
        with _on_device(dev):
            _lib.call("gae_mlp_predict", _ptr(X), ldx, n, d, hidden[0], hidden[1] if len(hidden) > 1 else 0, t,
                      _ptr(result.shift), _ptr(result.scale), _ptr(result.state), E, _ptr(out), _ptr(status), _stream())
        total = torch.zeros(n, t, dtype=torch.float64, device=dev)
        for k in range(E):
            total = total + out[k].double()
        return total / E
