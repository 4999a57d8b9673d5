#!/usr/bin/env python3
"""Ridge regression with a k-fold CV lambda path on the device (ops.ridge: gae_ridge_stats + gae_ridge_solve, K25) timed
with device events after warm-up on seeded data at three shapes with F = 5 folds and L = 13 lambdas: a molecule set of
ESOL's size (n = 1 128, d = 48), Pubmed's embedding (n = 19 717, d = 16) and the molecule features of embed_graphs
(n = 249 455, d = 48).  Beside it, alternating call by call and from the same inputs, the torch route a user had before:
per fold ``index_select`` -> ``.double()`` -> Gram matrix, per (fold, lambda) ``torch.linalg.cholesky`` +
``cholesky_solve``, the held-out error by a second product over the fold's rows.  The two launches of the kernel route
are also timed alone (the stats launch pair on its own buffers, the solve launch), the stats launch as a fraction of the
device copy rate bench.py measures at the same number of bytes.  The spread of every series is recorded: the machines
are shared.  Prints one JSON object (and writes it with --out).  No time or ratio is a pass condition.

    python tools/ridge_bench.py --out profiles/r15_ridge.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [("esol_features", 1128, 48), ("pubmed_z", 19717, 16), ("zinc_features", 249_455, 48)]
FOLDS, LAMBDAS = 5, [10.0 ** (e / 2.0) for e in range(-6, 7)]
FP64_MFMA_PEAK = 78.6e12          # v_mfma_f64_16x16x4_f64 (spec): 128 FLOP / clk / CU, 256 CUs, 2.4 GHz


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def series(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {"ms": float(np.median(xs)), "ms_min": float(xs.min()), "ms_max": float(xs.max()),
            "ms_p10": float(np.percentile(xs, 10)), "ms_p90": float(np.percentile(xs, 90)), "reps": int(xs.size)}


def torch_ridge(X, Y, fold, lambdas, F):
    """(coef [L, t, d] of the all-rows model, cv_sse [F, L, t]) by torch in fp64"""
    d, t = X.shape[1], Y.shape[1]
    parts, grams = [], []
    for f in range(F):
        idx = (fold == f).nonzero().reshape(-1)
        Xf, Yf = X.index_select(0, idx).double(), Y.index_select(0, idx).double()
        V = torch.cat([torch.ones(idx.shape[0], 1, dtype=torch.float64, device=X.device), Xf, Yf], 1)
        parts.append((Xf, Yf))
        grams.append(V.t() @ V)
    total = torch.stack(grams).sum(0)
    eye = torch.eye(d, dtype=torch.float64, device=X.device)
    sse = torch.empty(F, len(lambdas), t, dtype=torch.float64, device=X.device)
    coef = torch.empty(len(lambdas), t, d, dtype=torch.float64, device=X.device)
    for m in range(F + 1):
        S = total - grams[m] if m < F else total
        c, mu = S[0, 0], S[0, 1:] / S[0, 0]
        Cm = S[1:, 1:] - c * torch.outer(mu, mu)
        for l, lam in enumerate(lambdas):
            w = torch.cholesky_solve(Cm[:d, d:], torch.linalg.cholesky(Cm[:d, :d] + lam * eye))     # [d, t]
            b = mu[d:] - mu[:d] @ w
            if m < F:
                r = parts[m][1] - (parts[m][0] @ w + b)
                sse[m, l] = (r * r).sum(0)
            else:
                coef[l] = w.t()
    return coef, sse


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--case", choices=[c[0] for c in CASES], default=None, help="one shape only (kernel traces)")
    ap.add_argument("--no_torch", action="store_true", help="skip the torch route")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from gae_dgl_amd import _lib, ops
    from gae_dgl_amd.ops import _ptr, _stream
    dev = torch.device("cuda:0")
    rows = []
    for name, n, d in [c for c in CASES if a.case in (None, c[0])]:
        g = torch.Generator(device="cpu").manual_seed(n)
        X = torch.randn(n, d, generator=g)
        w = torch.randn(d, 1, generator=g) / d ** 0.5
        Y = (X @ w + 0.3 * torch.randn(n, 1, generator=g) + 2.0)
        fold = torch.empty(n, dtype=torch.int64)
        fold[torch.randperm(n, generator=g)] = torch.arange(n) % FOLDS
        X, Y, fold = X.to(dev), Y.to(dev), fold.to(dev)
        routes = {"ridge": lambda: ops.ridge(X, Y, LAMBDAS, folds=FOLDS, fold=fold)}
        if not a.no_torch:
            routes["torch_gram_cholesky"] = lambda: torch_ridge(X, Y, fold, LAMBDAS, FOLDS)
        times, out = {r: [] for r in routes}, {}
        for rep in range(a.warmup + a.reps):                              # alternating: every series sees the same neighbours
            for r, fn in routes.items():
                t = event_ms(lambda: out.__setitem__(r, fn()))
                if rep >= a.warmup:
                    times[r].append(t)
        row = {"case": name, "n": n, "d": d, "t": 1, "folds": FOLDS, "lambdas": len(LAMBDAS)}
        for r in routes:
            row[r] = series(times[r])
        res = out["ridge"]
        row["lam"], row["cv_r2_at_lam"] = res.lam, float(res.cv_r2[LAMBDAS.index(res.lam), 0])
        if "torch_gram_cholesky" in routes:
            row["ratio_torch_over_ridge"] = row["torch_gram_cholesky"]["ms"] / row["ridge"]["ms"]
            coef_t, sse_t = out["torch_gram_cholesky"]
            row["max_rel_coef_difference_vs_torch"] = float(((res.path_coef - coef_t).abs().max() / coef_t.abs().max()))
            row["max_rel_cv_sse_difference_vs_torch"] = float(((res.cv_sse - sse_t).abs() / sse_t.abs()).max())
        # ---- the two launches alone, on buffers of their own (the fold lists of the call above, rebuilt here)
        t_, W = 1, 2 + d
        order = torch.sort(fold, stable=True).indices.to(torch.int32)
        fold_ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.bincount(fold, minlength=FOLDS).cumsum(0)]
                             ).to(torch.int32)
        piv = torch.cat([X.mean(0), Y.mean(0)]).contiguous()
        ws = torch.empty(int(_lib.load().gae_ridge_workspace_bytes(n, d, t_, FOLDS)), dtype=torch.uint8, device=dev)
        stats = torch.empty(FOLDS, W * (W + 1) // 2, dtype=torch.float64, device=dev)
        status = torch.zeros(4, dtype=torch.int64, device=dev)
        lam = torch.tensor(LAMBDAS, dtype=torch.float64, device=dev)
        coef = torch.empty(FOLDS + 1, len(LAMBDAS), t_, d, dtype=torch.float64, device=dev)
        icpt = torch.empty(FOLDS + 1, len(LAMBDAS), t_, dtype=torch.float64, device=dev)
        sse = torch.empty(FOLDS, len(LAMBDAS), t_, dtype=torch.float64, device=dev)
        info = torch.empty(FOLDS + 1, len(LAMBDAS), dtype=torch.int32, device=dev)

        def run_stats():
            _lib.call("gae_ridge_stats", _ptr(X), d, _ptr(Y), t_, n, d, t_, _ptr(piv), _ptr(order), n, _ptr(fold_ptr), FOLDS,
                      _ptr(stats), _ptr(status), _ptr(ws), ws.numel(), _stream())

        def run_solve():
            _lib.call("gae_ridge_solve", _ptr(stats), d, t_, FOLDS, _ptr(piv), _ptr(lam), len(LAMBDAS), 0, _ptr(coef),
                      _ptr(icpt), _ptr(sse), _ptr(info), _ptr(status), _stream())
        t_stats = bench.time_launches(run_stats)
        t_solve = bench.time_launches(run_solve)
        row["status_clean"] = bool(int(status[0]) == 0 and int(status[1]) == 0)
        row["launch_bits_equal_to_call"] = bool(torch.equal(sse, res.cv_sse) and torch.equal(coef[FOLDS], res.path_coef))
        stream_bytes = n * (d + t_) * 4 + n * 4                           # X, Y and the row list, read once
        copy_gbs = bench.copy_bandwidth(stream_bytes, dev)
        row.update({"stats_launches_us": t_stats * 1e6, "solve_launch_us": t_solve * 1e6, "stats_stream_bytes": stream_bytes,
                    "stats_GBs": stream_bytes / t_stats / 1e9, "copy_GBs": copy_gbs,
                    "stats_fraction_of_copy_rate": stream_bytes / t_stats / 1e9 / copy_gbs,
                    "stats_fp64_flop": 2.0 * n * W * (W + 1) / 2,
                    "stats_fp64_matrix_peak_fraction": 2.0 * n * W * (W + 1) / 2 / t_stats / FP64_MFMA_PEAK})
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
        del X, Y, out
    result = {"what": "ops.ridge (gae_ridge_stats: the moment launch and the fold of its chunk partials; gae_ridge_solve: "
                      "one launch for the (F + 1) L models; fold lists, pivot, allocations and the one host read included) "
                      "against per-fold index_select -> double -> Gram, cholesky + cholesky_solve per (fold, lambda) and "
                      "a second product for the held-out error, in torch; seeded data, F = 5, L = 13, t = 1; device-event "
                      "timings of whole calls after warm-up, the series alternating call by call in one process; ms = "
                      "median.  stats_launches_us / solve_launch_us: the launches alone (bench.time_launches, HIP-graph "
                      "replay below 1 ms); stats_fraction_of_copy_rate = (X, Y and row list bytes) / time over the rate of "
                      "a device copy moving the same number of bytes (bench.copy_bandwidth, read + write counted); the "
                      "useful fp64 work is n W (W + 1) FLOP (upper triangle), the padded tiles do more",
              "reps": a.reps, "warmup": a.warmup, "rows": rows}
    text = json.dumps(result)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
