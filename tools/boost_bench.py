#!/usr/bin/env python3
"""Gradient boosting on the device (ops.boost: the column sort and edges in torch, gae_forest_bin, gae_boost_fit, K30) timed
with device events after a warm-up on seeded data at three shapes -- a molecule set of ESOL's size (n = 1 128, d = 48),
Pubmed's embedding (n = 19 717, d = 16) and the molecule features of embed_graphs (n = 249 455, d = 48) -- with 100
rounds, depth 4, 64 bins, 5 folds x 3 learning rates = 18 models side by side, for both objectives.  Reported: a whole
call, the gae_boost_fit launches alone (the same call, timed around the entry point) and from them the time per round,
beside launches per round x the time of one back-to-back launch measured here (5000 calls of gae_boost_predict on one
row through zero trees): what a round would cost if it were launch-bound.  Where sklearn imports,
``HistGradientBoostingRegressor`` / ``-Classifier`` (100 iterations, depth 4, 64 bins, learning rate 0.1, no early
stopping, 16 host threads) is fitted on the rows outside fold 0 and scored on fold 0: a different estimator of the same
family, its time and held-out R2 / accuracy beside ours (ours: pooled over the 5 folds at the chosen round).
``ops.forest``'s out-of-bag R2 on the same arrays stands beside the regression.  The spread of every series is recorded:
the machines are shared.  Prints one JSON object (and writes it with --out).  No time or ratio is a pass condition.

    python tools/boost_bench.py --out profiles/r20_boost.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [("esol_features", 1128, 48), ("pubmed_z", 19717, 16), ("zinc_features", 249_455, 48)]
ROUNDS, DEPTH, BINS, FOLDS, LRS = 100, 4, 64, 5, (0.3, 0.1, 0.03)


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--case", choices=[c[0] for c in CASES], default=None, help="one shape only (kernel traces)")
    ap.add_argument("--no_sklearn", action="store_true", help="skip the sklearn fits")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from gae_dgl_amd import _lib, ops
    from gae_dgl_amd.ops import _ptr, _stream
    from gae_dgl_amd.ops._heads import _default_fold
    try:
        if a.no_sklearn:
            raise ImportError("--no_sklearn")
        from sklearn.ensemble import HistGradientBoostingClassifier, HistGradientBoostingRegressor
        from threadpoolctl import threadpool_limits
    except ImportError as e:
        HistGradientBoostingRegressor, why_not = None, str(e)
    dev = torch.device("cuda:0")

    # one back-to-back launch: the entry point gae_boost_predict itself, one row through zero trees, 5000 in a row
    lib = _lib.load()
    one = torch.zeros(1, 2, device=dev)
    seen = torch.zeros(4, dtype=torch.int64, device=dev)
    sink = torch.empty(1, dtype=torch.float64, device=dev)
    args = (_ptr(one), 2, 1, 2, 0, 15, None, None, None, None, 0.0, _ptr(sink), _ptr(seen), _stream())

    def burst():
        for _ in range(5000):
            lib.gae_boost_predict(*args)
    burst()
    torch.cuda.synchronize()
    launch_us = sorted(event_ms(burst) / 5000 * 1e3 for _ in range(3))[1]

    inner = []
    plain_call = _lib.call

    def timed_call(name, *args):
        if name != "gae_boost_fit":
            return plain_call(name, *args)
        inner.append(event_ms(lambda: plain_call(name, *args)))
    rows = []
    for name, n, d in [c for c in CASES if a.case in (None, c[0])]:
        g = torch.Generator(device="cpu").manual_seed(n)
        X = torch.randn(n, d, generator=g)
        w = torch.randn(d, 1, generator=g) / d ** 0.5
        Y = (X @ w + 2.0 * (X[:, :1] > 0.25) * (X[:, 1:2] > 0).float() + 0.3 * torch.randn(n, 1, generator=g)).reshape(-1)
        labels = (Y > Y.median()).long()
        fold = _default_fold(n, FOLDS, 1)
        Xd, fd = X.to(dev), fold.to(dev)
        kw = dict(max_depth=DEPTH, max_bins=BINS, learning_rates=LRS, lambdas=(1.0,), folds=FOLDS, fold=fd)
        launches = 2 + 2 * DEPTH + (DEPTH - 1) + 1 + (DEPTH if n > ops.FOREST_SPLIT_ROWS else 0)
        row = {"case": name, "n": n, "d": d, "rounds": ROUNDS, "max_depth": DEPTH, "max_bins": BINS, "folds": FOLDS,
               "learning_rates": list(LRS), "models": (FOLDS + 1) * len(LRS), "launches_per_round": launches,
               "launch_us": launch_us, "launch_bound_round_ms": launches * launch_us / 1e3}
        for objective, yd in (("squared", Y.to(dev)), ("logistic", labels.to(dev))):
            out, call_ms, fit_ms = {}, [], []
            _lib.call = timed_call
            try:
                for rep in range(a.warmup + a.reps):
                    del inner[:]
                    t = event_ms(lambda: out.__setitem__("res", ops.boost(Xd, yd, objective, ROUNDS, **kw)))
                    if rep >= a.warmup:
                        call_ms.append(t)
                        fit_ms.append(inner[0])
            finally:
                _lib.call = plain_call
            res = out["res"]
            part = {"call": series(call_ms), "fit_launches": series(fit_ms),
                    "round_ms": float(np.median(fit_ms)) / (ROUNDS + 1), "best_round": res.best_round, "lr": res.lr,
                    "nodes": int(res.n_nodes.sum())}
            if objective == "squared":
                part.update(cv_r2=res.cv_r2, cv_rmse=res.cv_rmse)
                forest = ops.forest(Xd, yd, 100, max_depth=12, max_bins=BINS, seed=1)
                part["forest_oob_r2"] = float(forest.oob_r2[0])
                del forest
            else:
                part.update(cv_accuracy=res.cv_accuracy, cv_logloss=res.cv_logloss)
            if HistGradientBoostingRegressor is not None:
                Xh, yh, tr = X.numpy(), (Y if objective == "squared" else labels).numpy(), (fold != 0).numpy()
                cls = HistGradientBoostingRegressor if objective == "squared" else HistGradientBoostingClassifier
                ts = []
                with threadpool_limits(limits=16):
                    for _ in range(1 if n > 100_000 else 2):
                        t0 = time.perf_counter()
                        sk = cls(max_iter=ROUNDS, max_depth=DEPTH, max_bins=BINS, learning_rate=0.1, early_stopping=False,
                                 random_state=1).fit(Xh[tr], yh[tr])
                        ts.append((time.perf_counter() - t0) * 1e3)
                part["sklearn_one_model_fit"] = series(ts)
                part["sklearn_fold0_r2" if objective == "squared" else "sklearn_fold0_accuracy"] = float(sk.score(Xh[~tr], yh[~tr]))
            else:
                part["sklearn"] = f"not importable here ({why_not}): only our times"
            row[objective] = part
            del res, out
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
        del Xd
    result = {"what": "ops.boost (column sort and edges in torch, gae_forest_bin, gae_boost_fit, the selection on the host); "
                      "100 rounds, depth 4, 64 bins, 5 folds x 3 learning rates = 18 models per call; seeded data; "
                      "device-event timings of whole calls after warm-up; ms = median.  fit_launches: gae_boost_fit alone "
                      "inside the same calls; round_ms = fit_launches / 101 (100 rounds and the closing prologue).  "
                      "launch_bound_round_ms = launches_per_round x launch_us, launch_us = one of 5000 back-to-back "
                      "gae_boost_predict calls on one row through zero trees, measured in this run.  sklearn: ONE "
                      "HistGradientBoosting model (100 "
                      "iterations, depth 4, 64 bins, lr 0.1, 16 threads) on the rows outside fold 0, scored on fold 0, host "
                      "wall clock; ours trains 18 models and scores every fold",
              "reps": a.reps, "warmup": a.warmup, "rows": rows}
    text = json.dumps(result)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
