#!/usr/bin/env python3
"""The random forest head on the device (ops.forest: gae_forest_bin + gae_forest_fit + gae_forest_predict, K26) timed with
device events after warm-up on seeded data at three shapes with T = 100 trees, max_depth = 12, max_bins = 64: a molecule
set of ESOL's size (n = 1 128, d = 48), Pubmed's embedding (n = 19 717, d = 16) and the molecule features of embed_graphs
(n = 249 455, d = 48).  The whole call (edges, binning, growth, out-of-bag prediction, the host-side scores), `.predict`
on the training rows, and the three entry points alone on buffers of their own: their shares of a call.  Where sklearn
imports, ``RandomForestRegressor(n_estimators=100, max_depth=12, n_jobs=16, oob_score=True)`` is timed on the same arrays
(wall clock, host) with its out-of-bag R2 beside ours; where it does not, only our times are recorded and the result says
so.  The spread of every series is recorded: the machines are shared.  Prints one JSON object (and writes it with --out).
No time or ratio is a pass condition.

    python tools/forest_bench.py --out profiles/r16_forest.json
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [("esol_features", 1128, 48), ("pubmed_z", 19717, 16), ("zinc_features", 249_455, 48)]
TREES, DEPTH, BINS = 100, 12, 64


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--case", choices=[c[0] for c in CASES], default=None, help="one shape only (kernel traces)")
    ap.add_argument("--no_sklearn", action="store_true", help="skip the sklearn fit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from gae_dgl_amd import _lib, ops
    from gae_dgl_amd.ops import _ptr, _stream
    from gae_dgl_amd.ops._heads import _edges
    try:
        if a.no_sklearn:
            raise ImportError("--no_sklearn")
        from sklearn.ensemble import RandomForestRegressor
    except ImportError as e:
        RandomForestRegressor, why_not = None, str(e)
    dev = torch.device("cuda:0")
    rows = []
    for name, n, d in [c for c in CASES if a.case in (None, c[0])]:
        g = torch.Generator(device="cpu").manual_seed(n)
        X = torch.randn(n, d, generator=g)
        w = torch.randn(d, 1, generator=g) / d ** 0.5
        Y = (X @ w + 2.0 * (X[:, :1] > 0.25) + 0.3 * torch.randn(n, 1, generator=g)).reshape(-1)
        Xd, Yd = X.to(dev), Y.to(dev)
        kw = dict(max_depth=DEPTH, max_bins=BINS, seed=1)
        out, fit_ms, pred_ms = {}, [], []
        for rep in range(a.warmup + a.reps):
            t = event_ms(lambda: out.__setitem__("forest", ops.forest(Xd, Yd, TREES, **kw)))
            res = out["forest"]
            p = event_ms(lambda: res.predict(Xd))
            if rep >= a.warmup:
                fit_ms.append(t)
                pred_ms.append(p)
        row = {"case": name, "n": n, "d": d, "t": 1, "trees": TREES, "max_depth": DEPTH, "max_bins": BINS,
               "fit": series(fit_ms), "predict_training_rows": series(pred_ms), "nodes": int(res.n_nodes.sum()),
               "oob_r2": float(res.oob_r2[0]), "oob_rmse": float(res.oob_rmse[0])}
        # ---- the entry points alone, on buffers of their own
        lib = _lib.load()
        edges, n_edges = _edges(Xd, BINS)
        status = torch.zeros(4, dtype=torch.int64, device=dev)
        codes = torch.empty(n, d, dtype=torch.uint8, device=dev)
        M = min(2 ** (DEPTH + 1) - 1, 2 * n - 1)
        i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
        feature, tbin, left, count, n_nodes = i32(TREES, M), i32(TREES, M), i32(TREES, M), i32(TREES, M), i32(TREES)
        thr = torch.empty(TREES, M, dtype=torch.float32, device=dev)
        value = torch.empty(TREES, M, 1, dtype=torch.float64, device=dev)
        gain = torch.empty(TREES, M, dtype=torch.float64, device=dev)
        inbag = torch.empty(TREES, n, dtype=torch.uint8, device=dev)
        oob = torch.empty(n, 1, dtype=torch.float64, device=dev)
        ws = torch.empty(int(lib.gae_forest_workspace_bytes(n, d, 1, TREES, n, DEPTH, BINS)), dtype=torch.uint8, device=dev)
        piv = (ctypes.c_float * 1)(float(res.pivot[0]))
        exp = (ctypes.c_int32 * 1)(res.exponent[0])
        Y2 = Yd.reshape(n, 1).contiguous()

        def run_bin():
            _lib.call("gae_forest_bin", _ptr(Xd), d, n, d, None, n, _ptr(edges), _ptr(n_edges), BINS, _ptr(codes), _ptr(status),
                      _stream())

        def run_fit():
            _lib.call("gae_forest_fit", _ptr(codes), _ptr(n_edges), _ptr(edges), n, d, BINS, _ptr(Y2), 1, n, 1, None, piv, exp,
                      TREES, n, DEPTH, d, 1, _lib.FOREST_BOOTSTRAP, 1, _ptr(feature), _ptr(tbin), _ptr(thr), _ptr(left),
                      _ptr(count), _ptr(value), _ptr(gain), _ptr(n_nodes), M, _ptr(inbag), _ptr(status), _ptr(ws), ws.numel(),
                      _stream())

        def run_oob():
            _lib.call("gae_forest_predict", _ptr(Xd), d, n, d, 1, TREES, M, _ptr(feature), _ptr(thr), _ptr(left), _ptr(value),
                      _ptr(inbag), _ptr(oob), _ptr(status), _stream())
        parts = {}
        for label, fn in (("edges_torch", lambda: _edges(Xd, BINS)), ("bin", run_bin), ("fit", run_fit), ("oob_predict", run_oob)):
            ts = [event_ms(fn) for _ in range(a.warmup + a.reps)][a.warmup:]
            parts[label] = series(ts)
        row["entry_points"] = parts
        row["launch_bits_equal_to_call"] = bool(torch.equal(feature, res.feature) and torch.equal(value, res.value)
                                                and torch.equal(oob.isnan(), res.oob_prediction.isnan()))
        row["share_of_call"] = {k: v["ms"] / row["fit"]["ms"] for k, v in parts.items()}
        row["ws_MB"] = ws.numel() / 1e6
        if RandomForestRegressor is not None:
            Xh, Yh = X.numpy(), Y.numpy()
            ts = []
            for _ in range(1 if n > 100_000 else 2):
                t0 = time.perf_counter()
                sk = RandomForestRegressor(n_estimators=TREES, max_depth=DEPTH, n_jobs=16, oob_score=True, random_state=1).fit(Xh, Yh)
                ts.append((time.perf_counter() - t0) * 1e3)
            row["sklearn_fit"] = series(ts)
            row["sklearn_oob_r2"] = float(sk.oob_score_)
            t0 = time.perf_counter()
            sk.predict(Xh)
            row["sklearn_predict_ms"] = (time.perf_counter() - t0) * 1e3
            row["ratio_sklearn_over_forest_fit"] = row["sklearn_fit"]["ms"] / row["fit"]["ms"]
        else:
            row["sklearn"] = f"not importable here ({why_not}): only our times"
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
        del Xd, Yd, res, out, ws
    result = {"what": "ops.forest (column sort and edges in torch, gae_forest_bin, gae_forest_fit with one 32-byte read per "
                      "level, the out-of-bag gae_forest_predict, exactly rounded scores and importances on the host) and "
                      "ForestResult.predict on the training rows; T = 100, max_depth = 12, max_bins = 64, all features per "
                      "split, t = 1; seeded data; device-event timings of whole calls after warm-up; ms = median.  "
                      "entry_points: the same work through the C entry points on buffers of their own.  sklearn: "
                      "RandomForestRegressor(n_estimators=100, max_depth=12, n_jobs=16, oob_score=True) on the same arrays, "
                      "host wall clock (exact splits, not histograms: a different estimator of the same family)",
              "reps": a.reps, "warmup": a.warmup, "rows": rows}
    text = json.dumps(result)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
