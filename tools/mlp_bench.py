#!/usr/bin/env python3
"""The MLP regression head on the device (ops.mlp: gae_mlp_fit, K27) timed with device events after warm-up on seeded
data: a molecule set of ESOL's size (n = 1 128, d = 48) and Pubmed's embedding (n = 19 717, d = 16) with hidden = (100,),
5 folds x 4 configurations (24 models side by side), batch 200, 200 epochs; and the molecule features of embed_graphs
(n = 249 455, d = 48) for 10 epochs, one configuration, reported per epoch.  Whole ``ops.mlp`` calls, and the launches of
the same schedule alone (``bench.time_launches`` on gae_mlp_fit with buffers of its own).  Beside them the same schedule
in torch on the device, one model after another (``--torch_models K`` of the call's models are run and the time of all is
K's multiple: the models are alike), and, unless ``--no_sklearn``, ``sklearn.neural_network.MLPRegressor`` on 16 host
threads; the held-out R2 of each.  The comparison routes are plain torch / sklearn code that does not touch this
library: they are the same from any commit's tree.  The bound: the padded tiles' FLOPs of the longest model (the
all-rows one) at one CU's fp32 matrix rate, 256 FLOP / clk at 2.4 GHz -- derived from the guide's rates, not measured.
The spread of every series is recorded: the machines are shared.  Prints one JSON object (and writes it with --out).
No time or ratio is a pass condition.

    python tools/mlp_bench.py --out profiles/r17_mlp.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, n, d, epochs, lrs, alphas
CASES = [("esol_features", 1128, 48, 200, (1e-3, 1e-2), (1e-4, 1e-2)),
         ("pubmed_z", 19717, 16, 200, (1e-3, 1e-2), (1e-4, 1e-2)),
         ("zinc_features", 249_455, 48, 10, (1e-3,), (1e-4,))]
HIDDEN, FOLDS, BATCH = (100,), 5, 200
CU_FLOP_PER_CLK, CLOCK_HZ = 256, 2.4e9


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


def padded_flops_per_row(d, hidden, t):
    """forward, dW and dA products of one row on tiles of 16"""
    up = lambda v: (v + 15) // 16 * 16
    widths = [d] + list(hidden) + [t]
    total = 0
    for l in range(len(widths) - 1):
        total += 2 * up(widths[l]) * up(widths[l + 1]) * (3 if l > 0 else 2)
    return total


def r2_of(pred, y):
    return float(1.0 - ((pred - y) ** 2).sum() / ((y - y.mean()) ** 2).sum())


def torch_fit(Xs, Ys, hidden, lr, alpha, epochs, batch, seed):
    """the same schedule by torch on the device: Adam, L2 penalty alpha / B on the weights, a fresh permutation per epoch"""
    dev = Xs.device
    g = torch.Generator(device="cpu").manual_seed(seed)
    widths = [Xs.shape[1]] + list(hidden) + [Ys.shape[1]]
    layers = []
    for l in range(len(widths) - 1):
        layers.append(torch.nn.Linear(widths[l], widths[l + 1]))
        if l < len(widths) - 2:
            layers.append(torch.nn.ReLU())
    net = torch.nn.Sequential(*layers).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    weights = [m.weight for m in net if isinstance(m, torch.nn.Linear)]
    n = Xs.shape[0]
    for _ in range(epochs):
        perm = torch.randperm(n, generator=g).to(dev)
        for b0 in range(0, n, batch):
            idx = perm[b0:b0 + batch]
            opt.zero_grad(set_to_none=True)
            out = net(Xs[idx])
            loss = (0.5 * ((out - Ys[idx]) ** 2).sum() + 0.5 * alpha * sum((w ** 2).sum() for w in weights)) / idx.shape[0]
            loss.backward()
            opt.step()
    return net


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--case", choices=[c[0] for c in CASES], default=None, help="one shape only (kernel traces)")
    ap.add_argument("--torch_models", type=int, default=1, help="models of the call run by the torch route (0: skip it)")
    ap.add_argument("--no_sklearn", action="store_true", help="skip the sklearn fit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from gae_dgl_amd import _lib, ops
    from gae_dgl_amd.ops import _ptr, _stream
    from gae_dgl_amd.ops._heads import _fold_lists
    try:
        if a.no_sklearn:
            raise ImportError("--no_sklearn")
        from sklearn.neural_network import MLPRegressor
    except ImportError as e:
        MLPRegressor, why_not = None, str(e)
    dev = torch.device("cuda:0")
    rows = []
    for name, n, d, epochs, lrs, alphas in [c for c in CASES if a.case in (None, c[0])]:
        g = torch.Generator(device="cpu").manual_seed(n)
        X = torch.randn(n, d, generator=g)
        w = torch.randn(d, 1, generator=g) / d ** 0.5
        Y = ((X @ w).abs() + 0.5 * (X[:, :1] * X[:, 1:2]) + 0.3 * torch.randn(n, 1, generator=g)).reshape(-1)
        Xd, Yd = X.to(dev), Y.to(dev)
        kw = dict(lrs=lrs, alphas=alphas, epochs=epochs, batch_size=BATCH, folds=FOLDS, seed=1)
        out, call_ms = {}, []
        for rep in range(a.warmup + a.reps):
            t = event_ms(lambda: out.__setitem__("mlp", ops.mlp(Xd, Yd, HIDDEN, **kw)))
            if rep >= a.warmup:
                call_ms.append(t)
        res = out["mlp"]
        C, M = len(lrs) * len(alphas), res.info.numel()
        chosen = res.lrs.index(res.lr) * len(res.alphas) + res.alphas.index(res.alpha)
        row = {"case": name, "n": n, "d": d, "t": 1, "hidden": list(HIDDEN), "folds": FOLDS, "configurations": C, "models": M,
               "epochs": epochs, "batch_size": BATCH, "call": series(call_ms), "lr": res.lr, "alpha": res.alpha,
               "cv_r2": res.cv_r2[:, 0].tolist(), "cv_r2_chosen": float(res.cv_r2[chosen, 0])}
        # ---- the launches alone: one model on all rows, then the call's lists and models, on buffers of their own
        lib = _lib.load()
        per_launch = max(1, ops.MLP_LAUNCH_ROW_VISITS // n)
        V = torch.cat([Xd, Yd.reshape(n, 1)], 1)
        shift, std = V.mean(0).contiguous(), V.std(0, unbiased=False)
        scale = (1.0 / std).contiguous()
        Y2 = Yd.reshape(n, 1).contiguous()
        frows, fptr, _ = _fold_lists(None, n, FOLDS, 1, dev)
        ptr = fptr.cpu().tolist()

        def schedule(lists, train, evals, lr_l, al_l):
            Mm = len(train)
            all_rows = torch.cat(lists).contiguous()
            lens = [int(l.numel()) for l in lists]
            lp = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=dev)
            i32 = dict(dtype=torch.int32, device=dev)
            tr, ev = torch.tensor(train, **i32), torch.tensor(evals, **i32)
            lr = torch.tensor(lr_l, dtype=torch.float32, device=dev)
            al = torch.tensor(al_l, dtype=torch.float32, device=dev)
            sd = torch.arange(Mm, dtype=torch.int64, device=dev)
            loss = torch.empty(Mm, epochs, dtype=torch.float64, device=dev)
            sse = torch.empty(Mm, 1, dtype=torch.float64, device=dev)
            info = torch.empty(Mm, dtype=torch.int32, device=dev)
            status = torch.zeros(4, dtype=torch.int64, device=dev)
            ws = torch.empty(int(lib.gae_mlp_workspace_bytes(d, HIDDEN[0], 0, 1, Mm)), dtype=torch.uint8, device=dev)

            def run():
                for e0 in range(0, epochs, per_launch):
                    e1 = min(epochs, e0 + per_launch)
                    _lib.call("gae_mlp_fit", _ptr(Xd), d, _ptr(Y2), 1, n, d, HIDDEN[0], 0, 1, _ptr(shift), _ptr(scale),
                              _ptr(all_rows), all_rows.numel(), _ptr(lp), len(lists), _ptr(tr), _ptr(ev), _ptr(lr), _ptr(al),
                              _ptr(sd), Mm, BATCH, 0.9, 0.999, 1e-8, _lib.MLP_ADAM, 0.0,
                              _lib.MLP_SHUFFLE | (_lib.MLP_FINAL if e1 == epochs else 0), e0, e1, epochs, _ptr(loss), _ptr(sse),
                              _ptr(info), _ptr(status), _ptr(ws), ws.numel(), _stream())
            return run
        iters = 3 if n * epochs > 100_000 else 10
        one = schedule([frows], [0], [-1], [1e-2], [1e-4])
        t_one = bench.time_launches(one, iters=iters, warmup=1)
        lists, train, evals, lr_l, al_l = [], [], [], [], []
        for f in range(FOLDS):
            lists += [torch.cat([frows[:ptr[f]], frows[ptr[f + 1]:]]), frows[ptr[f]:ptr[f + 1]]]
        lists.append(frows)
        for c in range(C):
            for f in range(FOLDS + 1):
                train.append(2 * FOLDS if f == FOLDS else 2 * f)
                evals.append(-1 if f == FOLDS else 2 * f + 1)
                lr_l.append(lrs[c // len(alphas)]); al_l.append(alphas[c % len(alphas)])
        t_all = bench.time_launches(schedule(lists, train, evals, lr_l, al_l), iters=iters, warmup=1)
        steps = epochs * ((n + BATCH - 1) // BATCH)
        flops = padded_flops_per_row(d, HIDDEN, 1) * epochs * ((n + 31) // 32 * 32)
        bound_ms = flops / (CU_FLOP_PER_CLK * CLOCK_HZ) * 1e3
        row["launches"] = {"one_model_all_rows_ms": t_one * 1e3, "all_models_ms": t_all * 1e3, "launches_per_fit":
                           (epochs + per_launch - 1) // per_launch, "epochs_per_launch": per_launch,
                           "longest_launch_ms_estimate": t_all * 1e3 * min(per_launch, epochs) / epochs,
                           "steps_of_the_all_rows_model": steps, "us_per_step_one_model": t_one * 1e6 / steps,
                           "ms_per_epoch_one_model": t_one * 1e3 / epochs, "ms_per_epoch_all_models": t_all * 1e3 / epochs}
        row["bound"] = {"padded_flops_per_row": padded_flops_per_row(d, HIDDEN, 1), "one_model_ms": bound_ms,
                        "fraction_reached_one_model": bound_ms / (t_one * 1e3),
                        "fraction_reached_all_models": bound_ms / (t_all * 1e3),
                        "derived_from": "256 FLOP / clk / CU (4 SIMDs x 64) at 2.4 GHz; not measured"}
        row["share_of_call"] = {"launches": t_all * 1e3 / row["call"]["ms"]}
        # ---- the same schedule by torch, model after model (fold 0 of the chosen configuration first)
        Xs, Ys = (Xd - shift[:d]) * scale[:d], (Y2 - shift[d:]) * scale[d:]
        if a.torch_models > 0:
            ts, r2s = [], []
            for k in range(min(a.torch_models, FOLDS)):
                tr_rows, ev_rows = lists[2 * k].long(), lists[2 * k + 1].long()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                net = torch_fit(Xs[tr_rows], Ys[tr_rows], HIDDEN, res.lr, res.alpha, epochs, BATCH, k)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
                with torch.no_grad():
                    r2s.append(r2_of(net(Xs[ev_rows]) / scale[d:] + shift[d:], Y2[ev_rows]))
            per_model = float(np.median(ts))
            row["torch"] = {"models_run": len(ts), "per_model": series(ts), "all_models_ms": per_model * M,
                            "held_out_r2_of_the_folds_run": r2s,
                            "note": "wall clock with a device synchronisation; all_models_ms = the median model x models"}
            row["ratio_torch_all_models_over_call"] = per_model * M / row["call"]["ms"]
        if MLPRegressor is not None:
            from sklearn.model_selection import cross_val_score
            Xh, Yh = Xs.cpu().numpy(), Ys.reshape(-1).cpu().numpy()
            sk = MLPRegressor(hidden_layer_sizes=HIDDEN, learning_rate_init=res.lr, alpha=res.alpha, batch_size=BATCH,
                              max_iter=epochs, n_iter_no_change=epochs + 1, tol=0.0, random_state=1)
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                t0 = time.perf_counter()
                sk.fit(Xh, Yh)
                fit_ms = (time.perf_counter() - t0) * 1e3
                row["sklearn"] = {"one_model_all_rows_ms": fit_ms, "all_models_ms": fit_ms * M * (FOLDS - 1) / FOLDS,
                                  "note": "16 host threads at most; all_models_ms scales the all-rows fit to the call's "
                                          "models (fold models see (F - 1) / F of the rows)"}
                if n <= 20_000:
                    t0 = time.perf_counter()
                    cv = cross_val_score(sk, Xh, Yh, cv=FOLDS, scoring="r2", n_jobs=5)
                    row["sklearn"]["cv_r2_mean"] = float(cv.mean())
                    row["sklearn"]["cv_5_fits_on_5_processes_ms"] = (time.perf_counter() - t0) * 1e3
            row["ratio_sklearn_all_models_over_call"] = row["sklearn"]["all_models_ms"] / row["call"]["ms"]
        else:
            row["sklearn"] = f"not importable here ({why_not}): only our times and torch's"
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
        del Xd, Yd, res, out
    result = {"what": "ops.mlp (fold lists and scaling in torch, gae_mlp_fit in launches of at most MLP_LAUNCH_ROW_VISITS row "
                      "visits per model with one status read each, one read of the tables) with hidden = (100,), 5 folds, "
                      "batch 200, Adam; seeded data; device-event timings of whole calls after warm-up; ms = median.  "
                      "launches: gae_mlp_fit alone through bench.time_launches, for one all-rows model and for the call's "
                      "models.  bound: the padded tiles' FLOPs at one CU's fp32 matrix rate, derived from the guide's "
                      "rates.  torch: the same schedule on the device, model after model.  sklearn: MLPRegressor with the "
                      "chosen (lr, alpha) on the standardised arrays, host wall clock",
              "reps": a.reps, "warmup": a.warmup, "launch_row_visits": ops.MLP_LAUNCH_ROW_VISITS, "rows": rows}
    text = json.dumps(result)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
