#!/usr/bin/env python3
"""k-means on the device (ops.kmeans: gae_kmeans_step, four launches per Lloyd iteration, one host read at the end)
timed with device events after warm-up at a fixed iteration count, on seeded overlapping blobs, at three sizes:
n = 19 717, d = 16, k = 3 (Pubmed's embedding and classes), n = 200 000, d = 16, k = 64, and n = 249 455, d = 48, k = 256
(the molecule features of embed_graphs).  Beside it, alternating call by call and from the same initial centres, the
route a user had before: ``torch.cdist`` -> ``argmin`` -> ``index_add_`` for the same number of iterations, which forms
the n x k distance matrix.  The assignment alone (ops.kmeans_assign, one launch) is timed as well.  The spread of every
series is recorded: the machines are shared.
Prints one JSON object (and writes it with --out).  No time or ratio is a pass condition.

    python tools/kmeans_bench.py --out profiles/r13_kmeans.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [("pubmed_z", 19717, 16, 3), ("n200k", 200_000, 16, 64), ("zinc_features", 249_455, 48, 256)]


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
            "ms_p10": float(np.percentile(xs, 10)), "ms_p90": float(np.percentile(xs, 90))}


def blobs(n, d, k, noise, seed, dev):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    centres = torch.randint(-16, 17, (k, d), generator=gen).float() / 4
    X = centres[torch.arange(n) % k] + noise * torch.randn(n, d, generator=gen)
    return X.to(dev)


def torch_lloyd(X, C0, iters):
    """the same iterations with stock torch ops: the n x k distances, float atomics in index_add_"""
    C = C0.clone()
    k = C.shape[0]
    ones = torch.ones(X.shape[0], device=X.device)
    for _ in range(iters):
        labels = torch.cdist(X, C).argmin(1)
        sums = torch.zeros_like(C).index_add_(0, labels, X)
        counts = torch.zeros(k, device=X.device).index_add_(0, labels, ones)
        C = torch.where(counts[:, None] > 0, sums / counts.clamp(min=1)[:, None], C)
    return labels, C


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10, help="Lloyd iterations per timed call, both routes")
    ap.add_argument("--noise", type=float, default=6.0,
                    help="blob noise: large enough that no run converges before --iters (native_n_iter in the output says)")
    ap.add_argument("--case", choices=[c[0] for c in CASES], default=None, help="one size only (kernel traces)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from gae_dgl_amd import ops
    dev = torch.device("cuda:0")
    rows = []
    for name, n, d, k in [c for c in CASES if a.case in (None, c[0])]:
        X = blobs(n, d, k, a.noise, 0, dev)
        C0 = X[:k].clone()

        def native():
            return ops.kmeans(X, k, init=C0, tol=0, max_iter=a.iters, check_every=a.iters, check_finite=False)

        def stock():
            out = torch_lloyd(X, C0, a.iters)
            out[0][:1].cpu()                                      # one host read, as the native call ends in
            return out
        for _ in range(a.warmup):
            res = native()
            labels_t, _ = stock()
        torch.cuda.synchronize()
        t_native, t_stock, t_assign = [], [], []
        for _ in range(a.reps):                                   # alternating: both series see the same neighbours
            t_native.append(event_ms(native))
            t_stock.append(event_ms(stock))
        for _ in range(a.warmup + a.reps):
            t_assign.append(event_ms(lambda: ops.kmeans_assign(X, C0)))
        row = {"case": name, "n": n, "d": d, "k": k, "iters": a.iters, "native_n_iter": res.n_iter,
               "native_converged": res.converged, "kmeans": series(t_native), "torch_cdist_argmin_index_add": series(t_stock),
               "assign_alone": series(t_assign[a.warmup:]), "distance_matrix_bytes": 4 * n * k,
               "labels_equal_fraction": float((res.labels.long() == labels_t).double().mean())}
        row["ratio_torch_over_kmeans"] = row["torch_cdist_argmin_index_add"]["ms"] / row["kmeans"]["ms"]
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    result = {"what": "ops.kmeans (gae_kmeans_step x iters, tol = 0, one status read at the end) against torch.cdist -> "
                      "argmin -> index_add_ for the same number of iterations from the same centres, on seeded blobs "
                      "(centres integers / 4, noise as given); device-event timings of whole calls after warm-up, the "
                      "two series alternating call by call in one process; ms = median; assign_alone = one "
                      "ops.kmeans_assign call (its allocation included)",
              "noise": a.noise, "reps": a.reps, "rows": rows}
    text = json.dumps(result)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
