#!/usr/bin/env python3
"""Principal components on the device (ops.pca: gae_ridge_stats + gae_pca_solve, K31; gae_pca_transform) timed with
device events after warm-up on seeded data at four shapes: a molecule set of ESOL's size (n = 1 128, d = 48), Pubmed's
embedding (n = 19 717, d = 16), the molecule features of embed_graphs (n = 249 455, d = 48) and n = 19 717 at d = 128,
the solver's worst case.  Beside it, alternating call by call and from the same input, the torch route a user had
before: fp64 centring, ``X.T @ X``, ``torch.linalg.eigh``, ``X @ V``.  gae_pca_solve and gae_pca_transform (k = 2 and k
= d) are also timed alone, the projection as a fraction of the device copy rate bench.py measures at the same number of
bytes.  Last, a 1 000-iteration ``ops.tsne`` of a Cora-sized embedding (n = 2 708, d = 16) from the Philox start and from
``init="pca"``, with the final KL of both.  The spread of every series is recorded: the machines are shared.  Prints one
JSON object (and writes it with --out).  No time or ratio is a pass condition.

    python tools/pca_bench.py --out profiles/r21_pca.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [("esol_features", 1128, 48), ("pubmed_z", 19717, 16), ("zinc_features", 249_455, 48), ("wide_128", 19717, 128)]


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


def torch_pca(X, k):
    """(values [k] descending, components [k, d], scores fp64 [n, k]) by torch in fp64"""
    Xc = X.double()
    Xc = Xc - Xc.mean(0)
    C = Xc.t() @ Xc / (X.shape[0] - 1)
    w, V = torch.linalg.eigh(C)
    V = V.flip(1)[:, :k]
    return w.flip(0)[:k], V.t(), Xc @ V


def clustered(n, d, classes, gen):
    centres = 3.0 * torch.randn(classes, d, generator=gen)
    return centres[torch.randint(0, classes, (n,), generator=gen)] + torch.randn(n, d, generator=gen)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tsne_iters", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from gae_dgl_amd import _lib, ops
    from gae_dgl_amd.ops import _ptr, _stream
    dev = torch.device("cuda:0")
    rows = []
    for name, n, d in CASES:
        g = torch.Generator(device="cpu").manual_seed(n + d)
        X = (torch.randn(n, d, generator=g) * (0.2 + 3.0 * torch.rand(d, generator=g))) @ \
            (torch.eye(d) + 0.3 * torch.randn(d, d, generator=g))
        X = X.to(dev)
        routes = {"pca": lambda: ops.pca(X), "torch_eigh": lambda: torch_pca(X, d)}
        times, out = {r: [] for r in routes}, {}
        for rep in range(a.warmup + a.reps):                              # alternating: every series sees the same neighbours
            for r, fn in routes.items():
                t = event_ms(lambda: out.__setitem__(r, fn()))
                if rep >= a.warmup:
                    times[r].append(t)
        res = out["pca"]
        w_t, V_t, Z_t = out["torch_eigh"]
        row = {"case": name, "n": n, "d": d, "n_sweeps": res.n_sweeps}
        for r in routes:
            row[r] = series(times[r])
        row["ratio_torch_over_pca"] = row["torch_eigh"]["ms"] / row["pca"]["ms"]
        row["max_rel_value_difference_vs_torch"] = float(((res.explained_variance - w_t).abs() / w_t.abs().max()).max())
        again = ops.pca(X)
        row["same_bits_run_to_run"] = bool(torch.equal(again.components, res.components) and
                                           torch.equal(again.explained_variance, res.explained_variance))
        # ---- the launches alone, on buffers of their own
        W = d + 2
        piv = torch.cat([X.mean(0), X.mean(0)[:1]]).contiguous()
        lib = _lib.load()
        ws = torch.empty(max(lib.gae_ridge_workspace_bytes(n, d, 1, 1), lib.gae_pca_workspace_bytes(d)), dtype=torch.uint8, device=dev)
        stats = torch.empty(W * (W + 1) // 2, dtype=torch.float64, device=dev)
        rstatus = torch.zeros(4, dtype=torch.int64, device=dev)
        status = torch.zeros(8, dtype=torch.int64, device=dev)
        mean = torch.empty(d, dtype=torch.float64, device=dev)
        values = torch.empty(d, dtype=torch.float64, device=dev)
        comps = torch.empty(d, d, dtype=torch.float64, device=dev)
        _lib.call("gae_ridge_stats", _ptr(X), d, _ptr(X), d, n, d, 1, _ptr(piv), None, n, None, 1, _ptr(stats), _ptr(rstatus),
                  _ptr(ws), ws.numel(), _stream())

        def run_solve():
            _lib.call("gae_pca_solve", _ptr(stats), d, 1, _ptr(piv), n, d, 0, _ptr(mean), _ptr(values), _ptr(comps),
                      _ptr(status), _ptr(ws), ws.numel(), _stream())
        t_solve = bench.time_launches(run_solve, iters=10, warmup=2)
        row["solve_launch_us"] = t_solve * 1e6
        row["launch_bits_equal_to_call"] = bool(torch.equal(comps, res.components) and torch.equal(values, res.explained_variance))
        rounds = int(status[1]) * (d + (d & 1) - 1)
        row["solve_rounds"] = rounds
        row["solve_us_per_round"] = t_solve * 1e6 / max(rounds, 1)
        for k in sorted({min(2, d), d}):
            Z = torch.empty(n, k, dtype=torch.float32, device=dev)

            def run_transform():
                _lib.call("gae_pca_transform", _ptr(X), d, n, d, None, n, _ptr(mean), _ptr(comps), None, k, 0, _ptr(Z), k,
                          _ptr(status), _stream())
            t_tr = bench.time_launches(run_transform)
            nbytes = n * d * 4 + n * k * 4                               # X read once, Z written once
            copy_gbs = bench.copy_bandwidth(nbytes, dev)
            row[f"transform_k{k}"] = {"launch_us": t_tr * 1e6, "bytes": nbytes, "GBs": nbytes / t_tr / 1e9, "copy_GBs": copy_gbs,
                                      "fraction_of_copy_rate": nbytes / t_tr / 1e9 / copy_gbs}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
        del X, out
    # ---- t-SNE of a Cora-sized embedding from both starts
    g = torch.Generator(device="cpu").manual_seed(2708)
    Zc = clustered(2708, 16, 7, g).to(dev)
    tsne = {}
    for label, init in (("philox", None), ("pca", "pca")):
        ops.tsne(Zc, n_iter=20, init=init)                                # warm-up
        ts, res = [], None
        for _ in range(a.reps):
            ts.append(event_ms(lambda: tsne.__setitem__("res", ops.tsne(Zc, n_iter=a.tsne_iters, init=init))))
        res = tsne.pop("res")
        tsne[label] = dict(series(ts), kl_divergence=res.kl_divergence, n_iter=res.n_iter)
    result = {"what": "ops.pca (gae_ridge_stats, gae_pca_solve in one block, the pivot, allocations and the one host read "
                      "included; all d components) against fp64 centring -> X^T X -> torch.linalg.eigh -> X V in torch; "
                      "seeded data; device-event timings of whole calls after warm-up, the series alternating call by "
                      "call in one process; ms = median.  solve_launch_us / transform_k*: the launches alone "
                      "(bench.time_launches, HIP-graph replay below 1 ms); fraction_of_copy_rate = (X read + Z written) / "
                      "time over the rate of a device copy moving the same number of bytes (bench.copy_bandwidth).  tsne: "
                      "n = 2 708, d = 16, 7 seeded clusters, whole ops.tsne calls",
              "reps": a.reps, "warmup": a.warmup, "rows": rows, "tsne": tsne}
    text = json.dumps(result)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
