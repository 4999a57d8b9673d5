#!/usr/bin/env python3
"""Multinomial logistic regression with a k-fold CV lambda path on the device (ops.logreg: gae_ridge_stats +
gae_logreg_factor, then gae_logreg_pass + gae_logreg_update per pass, K28) timed with device events after a warm-up on
seeded data at the three shapes of the other heads, each with F = 5 folds and L = 13 lambdas (78 models side by side): a
molecule set of ESOL's size (n = 1 128, d = 48, c = 2), Pubmed's embedding (n = 19 717, d = 16, c = 3) and the molecule
features of embed_graphs (n = 249 455, d = 48, c = 2).  Reported per shape: the whole call; the passes per model and per
second; gae_logreg_pass alone (every model active, on buffers of its own) as a fraction of the fp32 matrix peak and of
the device copy rate; the same objective by torch.optim.LBFGS on the device, ONE fold model timed and multiplied by the
call's models; sklearn's LogisticRegression on the host when it is importable.  The spread of every series is recorded:
the machines are shared.  Prints one JSON object (and writes it with --out).  No time or ratio is a pass condition.

    python tools/logreg_bench.py --out profiles/r18_logreg.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [("esol_features", 1128, 48, 2), ("pubmed_z", 19717, 16, 3), ("zinc_features", 249_455, 48, 2)]
FOLDS, LAMBDAS = 5, [10.0 ** (e / 2.0) for e in range(-6, 7)]
FP32_MFMA_PEAK = 157.3e12         # v_mfma_f32_16x16x4_f32 (spec): 256 FLOP / clk / CU, 256 CUs, 2.4 GHz


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def series(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {"ms": float(np.median(xs)), "ms_min": float(xs.min()), "ms_max": float(xs.max()), "reps": int(xs.size)}


def make(n, d, c, seed):
    """overlapping Gaussian classes, features on different scales"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    centres = torch.randn(c, d, generator=g) * (2.0 / (2.0 * d) ** 0.5)
    y = torch.randint(0, c, (n,), generator=g)
    X = (centres[y] + torch.randn(n, d, generator=g)) * torch.exp(torch.rand(d, generator=g) * 3.0 - 0.7) + 5.0
    fold = torch.empty(n, dtype=torch.int64)
    fold[torch.randperm(n, generator=g)] = torch.arange(n) % FOLDS
    return X, y, fold


def torch_lbfgs(X, y, c, lam, steps=100):
    """one model by torch.optim.LBFGS on the device, fp32, standardised features (LBFGS needs them; ours does not)"""
    Xs = (X - X.mean(0)) / X.std(0)
    W = torch.zeros(c, X.shape[1] + 1, device=X.device, requires_grad=True)
    opt = torch.optim.LBFGS([W], max_iter=steps, tolerance_grad=1e-5, tolerance_change=1e-9, line_search_fn="strong_wolfe")

    def closure():
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(Xs @ W[:, 1:].t() + W[:, 0], y, reduction="sum") + 0.5 * lam * (W[:, 1:] ** 2).sum()
        loss.backward()
        return loss
    opt.step(closure)
    return W.detach()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--case", choices=[c[0] for c in CASES], default=None, help="one shape only")
    ap.add_argument("--no_torch", action="store_true", help="skip the torch and sklearn routes")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from gae_dgl_amd import _lib, ops
    from gae_dgl_amd.ops import _ptr, _stream
    dev = torch.device("cuda:0")
    L, M = len(LAMBDAS), (FOLDS + 1) * len(LAMBDAS)
    rows = []
    for name, n, d, c in [s for s in CASES if a.case in (None, s[0])]:
        Xh, yh, foldh = make(n, d, c, n)
        X, y, fold = Xh.to(dev), yh.to(dev), foldh.to(dev)
        times, res = [], None
        for rep in range(a.warmup + a.reps):
            holder = {}
            t = event_ms(lambda: holder.__setitem__("r", ops.logreg(X, y, LAMBDAS, folds=FOLDS, fold=fold)))
            res = holder["r"]
            if rep >= a.warmup:
                times.append(t)
        row = {"case": name, "n": n, "d": d, "c": c, "folds": FOLDS, "lambdas": L, "models": M, "logreg": series(times)}
        n_iter = res.n_iter.cpu().numpy()
        row.update({"lam": res.lam, "cv_accuracy_at_lam": float(res.cv_accuracy[LAMBDAS.index(res.lam)]),
                    "cv_logloss_at_lam": float(res.cv_logloss[LAMBDAS.index(res.lam)]), "passes_max": int(n_iter.max()),
                    "passes_mean_per_model": float(n_iter.mean()), "converged_models": int(res.converged.sum()),
                    "model_passes_per_second": float(n_iter.sum()) / (row["logreg"]["ms"] * 1e-3)})
        # ---- gae_logreg_pass alone: every model active (a fresh factor call), V = 0, buffers of its own
        order = torch.sort(fold, stable=True).indices.to(torch.int32)
        fold_ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.bincount(fold, minlength=FOLDS).cumsum(0)]
                             ).to(torch.int32)
        piv = X.index_select(0, order.long()).mean(0).contiguous()
        Wr = d + 2
        stats = torch.empty(FOLDS, Wr * (Wr + 1) // 2, dtype=torch.float64, device=dev)
        rws = torch.empty(int(_lib.load().gae_ridge_workspace_bytes(n, d, 1, FOLDS)), dtype=torch.uint8, device=dev)
        nbytes = int(_lib.load().gae_logreg_workspace_bytes(n, d, c, FOLDS, L, M))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        rstatus, status = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
        lam = torch.tensor(LAMBDAS, dtype=torch.float64, device=dev)
        coef = torch.empty(M, c, d, dtype=torch.float64, device=dev)
        icpt = torch.empty(M, c, dtype=torch.float64, device=dev)
        info, nit, conv = (torch.empty(M, dtype=torch.int32, device=dev) for _ in range(3))
        y32, ycol = y.to(torch.int32), y.float().reshape(n, 1)
        pr = torch.cat([piv, piv.new_zeros(1)])
        _lib.call("gae_ridge_stats", _ptr(X), d, _ptr(ycol), 1, n, d, 1, _ptr(pr), _ptr(order), n, _ptr(fold_ptr), FOLDS,
                  _ptr(stats), _ptr(rstatus), _ptr(rws), rws.numel(), _stream())
        _lib.call("gae_logreg_factor", _ptr(stats), d, c, FOLDS, _ptr(lam), L, n, M, _ptr(coef), _ptr(icpt), _ptr(info),
                  _ptr(nit), _ptr(conv), _ptr(status), _ptr(ws), nbytes, _stream())

        def run_pass():
            _lib.call("gae_logreg_pass", _ptr(X), d, _ptr(y32), n, d, c, _ptr(piv), _ptr(order), n, _ptr(fold_ptr), FOLDS, L, M,
                      0, M, 0, None, None, _ptr(status), _ptr(ws), nbytes, _stream())

        def run_update():                                              # iteration 1 of 2^30: no model stops, V moves
            _lib.call("gae_logreg_update", d, c, FOLDS, _ptr(lam), L, n, M, 0, M, 1, 1 << 30, 0.0, _ptr(piv), _ptr(coef),
                      _ptr(icpt), _ptr(info), _ptr(nit), _ptr(conv), _ptr(status), _ptr(ws), nbytes, _stream())
        t_pass = bench.time_launches(run_pass)
        t_update = bench.time_launches(lambda: (run_pass(), run_update())) - t_pass
        tiles = -(-M // 4)
        train_rows = n * (FOLDS * (FOLDS - 1) / FOLDS + 1) * L         # rows x models that use them
        flop = 4.0 * c * (d + 1) * train_rows                          # logits + gradient, unpadded
        stream_bytes = n * (d * 4 + 8) * tiles                         # X, row list and labels once per model tile
        copy_gbs = bench.copy_bandwidth(n * (d * 4 + 8), dev)
        row.update({"pass_launch_us": t_pass * 1e6, "update_launch_us": t_update * 1e6, "pass_useful_flop": flop,
                    "pass_fp32_matrix_peak_fraction": flop / t_pass / FP32_MFMA_PEAK, "pass_stream_bytes": stream_bytes,
                    "pass_GBs": stream_bytes / t_pass / 1e9, "copy_GBs": copy_gbs,
                    "pass_fraction_of_copy_rate": stream_bytes / t_pass / 1e9 / copy_gbs,
                    "status_clean": bool(int(status[2]) == 0 and int(rstatus[0]) == 0)})
        if not a.no_torch:
            tr = (fold != 0).nonzero().reshape(-1)
            Xt, yt = X.index_select(0, tr), y.index_select(0, tr)
            ts = []
            for rep in range(a.warmup + a.reps):
                t = event_ms(lambda: torch_lbfgs(Xt, yt, c, res.lam))
                if rep >= a.warmup:
                    ts.append(t)
            row["torch_lbfgs_one_fold_model"] = series(ts)
            row["torch_lbfgs_scaled_to_the_calls_models_ms"] = row["torch_lbfgs_one_fold_model"]["ms"] * M
            row["ratio_torch_scaled_over_logreg"] = row["torch_lbfgs_scaled_to_the_calls_models_ms"] / row["logreg"]["ms"]
            try:
                from sklearn.linear_model import LogisticRegression
                import sklearn
                Xn, yn = Xt.cpu().numpy(), yt.cpu().numpy()
                t0 = time.perf_counter()
                LogisticRegression(C=1.0 / res.lam, max_iter=1000).fit(Xn, yn)
                row["sklearn_one_fold_model_ms"] = (time.perf_counter() - t0) * 1e3
                row["sklearn_version"] = sklearn.__version__
            except ImportError:
                row["sklearn_one_fold_model_ms"] = None
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
        del X, y, res
    result = {"what": "ops.logreg (gae_ridge_stats + gae_logreg_factor once, gae_logreg_pass + gae_logreg_update per pass "
                      "for all (F + 1) L = 78 models, the evaluation pass, fold lists, pivot, allocations, the status reads "
                      "every 8 passes and the one read of the tables included); seeded overlapping Gaussian classes, F = 5, "
                      "L = 13, tol = 1e-4; device-event timings of whole calls after a warm-up, ms = median.  "
                      "pass_launch_us / update_launch_us: the launches alone with every model active (bench.time_launches, "
                      "HIP-graph replay below 1 ms; the update as the difference of pass + update and pass).  "
                      "pass_useful_flop = 4 c (d + 1) per (model, training row), the padded tiles do more; "
                      "pass_stream_bytes = (X, row list, labels) once per tile of 4 models over the rate of a device copy "
                      "moving one such stream (bench.copy_bandwidth).  torch_lbfgs: torch.optim.LBFGS (strong Wolfe, 100 "
                      "iterations at most, fp32, standardised features) on ONE fold model at the chosen lambda, multiplied "
                      "by the call's models; sklearn: LogisticRegression(C = 1 / lambda) on the host for the same model",
              "reps": a.reps, "warmup": a.warmup, "rows": rows}
    text = json.dumps(result)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
