#!/usr/bin/env python3
"""The spectral-embedding baseline on the device (ops.spectral_embedding, K32) timed with device events after a warm-up
at three shapes: a Cora-sized graph (n = 2 708), a Pubmed-sized one (n = 19 717, 88 648 directed edges) and a synthetic
graph of 2.10^5 nodes of mean degree 10, all at k = 16, b = 32, degree 8, tol 1e-8.  Per shape: the whole call, its outer
iterations and block products; every kernel alone on buffers of its own (bench.time_launches) and its share of the call;
gae_spectral_spmm against its byte bound (the gather 8 b nnz, the streams 8 b n in and out, the index bytes) at the
measured device copy rate, warm and MALL-cold; gae_spectral_gram and gae_spectral_rotate against the copy rate and the
fp64 matrix peak.  Beside it two routes the change does not touch: the same schedule in torch on the device
(torch.sparse.mm in fp64, torch.linalg.cholesky / eigh on the b x b matrices) and scipy.sparse.linalg.eigsh(which="LA") on
the host -- a different algorithm (implicitly restarted Lanczos), named as such.  The spread of every series is
recorded: the machines are shared.  Prints one JSON object (and writes it with --out).  No time or ratio is a pass
condition.

    python tools/spectral_bench.py --out profiles/r22_spectral.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, B, DEGREE, TOL = 16, 32, 8, 1e-8
FP64_MATRIX_PEAK = 78.6e12      # MI355X spec, fp64 matrix FLOP/s
CASES = [("cora_sized", 2708, 5278), ("pubmed_sized", 19717, 44324), ("synthetic_200k", 200_000, 1_000_000)]


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


def random_graph(n, pairs, seed):
    """(src, dst) of `pairs` distinct undirected pairs, both directions listed"""
    rng = np.random.default_rng(seed)
    u, v = rng.integers(0, n, 2 * pairs), rng.integers(0, n, 2 * pairs)
    keep = u != v
    key = np.unique(np.minimum(u, v)[keep] * n + np.maximum(u, v)[keep])
    key = key[rng.permutation(key.shape[0])[:pairs]]
    u, v = key // n, key % n
    return np.concatenate([u, v]), np.concatenate([v, u])


def torch_route(S, n, seed, max_iter=200):
    """the same schedule in torch: (values [K], n_iter) -- sparse fp64 products, cholesky and eigh of the b x b matrices,
    the same filter"""
    gen = torch.Generator(device=S.device).manual_seed(seed)
    V = torch.randn(n, B, dtype=torch.float64, device=S.device, generator=gen)
    for it in range(1, max_iter + 1):
        AV = torch.sparse.mm(S, V)
        L = torch.linalg.cholesky(V.t() @ V)
        Hp = torch.linalg.solve_triangular(L, torch.linalg.solve_triangular(L, V.t() @ AV, upper=False).t(), upper=False)
        w, W = torch.linalg.eigh((Hp + Hp.t()) * 0.5)
        w, W = w.flip(0), W.flip(1)
        T = torch.linalg.solve_triangular(L.t(), W, upper=True)
        V, AV = V @ T, AV @ T
        res = (AV - V * w[None, :]).norm(dim=0)
        if bool((res[:K] <= TOL).all()) or it == max_iter:                # one host read per iteration, as check_every = 1
            return w[:K], it
        a = max(min(float(w[-1]), float(w[K - 1]) - 0.02), -0.5)
        e, c = (a + 1.0) * 0.5, (a - 1.0) * 0.5
        s1 = e / (float(w[0]) - c)
        s = s1
        prev, cur = V, (s1 / e) * (torch.sparse.mm(S, V) - c * V)
        for _ in range(2, DEGREE + 1):
            s2 = 1.0 / (2.0 / s1 - s)
            prev, cur = cur, (2.0 * s2 / e) * (torch.sparse.mm(S, cur) - c * cur) - (s * s2) * prev
            s = s2
        V = cur


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no_scipy", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    import gae_dgl_amd as G
    from gae_dgl_amd import _lib, ops
    from gae_dgl_amd.ops import _ptr, _stream
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rows = []
    for name, n, pairs in CASES:
        src, dst = random_graph(n, pairs, n)
        g = G.DGLGraph((src, dst), num_nodes=n).to(dev)
        indptr, indices = g.csr()
        nnz = int(indices.shape[0])
        out = {}
        routes = {"spectral": lambda: ops.spectral_embedding(g, K, oversample=B - K, degree=DEGREE, tol=TOL)}
        deg = torch.bincount(torch.from_numpy(dst), minlength=n).double()
        sc = torch.where(deg > 0, deg.rsqrt(), torch.zeros_like(deg))
        idx = torch.from_numpy(np.stack([dst, src]))
        S = torch.sparse_coo_tensor(idx, sc[dst] * sc[src], (n, n)).coalesce().to_sparse_csr().to(dev)
        routes["torch_same_schedule"] = lambda: torch_route(S, n, 0)
        times = {r: [] for r in routes}
        for rep in range(a.warmup + a.reps):                              # alternating: every series sees the same neighbours
            for r, fn in routes.items():
                t = event_ms(lambda: out.__setitem__(r, fn()))
                if rep >= a.warmup:
                    times[r].append(t)
        res = out["spectral"]
        row = {"case": name, "n": n, "nnz": nnz, "k": K, "b": B, "degree": DEGREE, "tol": TOL, "n_iter": res.n_iter,
               "n_spmm": res.n_spmm, "converged": bool(res.converged), "residual_max": float(res.residuals.max()),
               "max_degree": int(deg.max())}
        for r in routes:
            row[r] = series(times[r])
        row["torch_n_iter"] = int(out["torch_same_schedule"][1])
        row["max_value_difference_vs_torch"] = float((res.values - out["torch_same_schedule"][0]).abs().max())
        again = routes["spectral"]()
        row["same_bits_run_to_run"] = bool(torch.equal(again.vectors, res.vectors) and torch.equal(again.values, res.values))
        if not a.no_scipy:
            import scipy.sparse as sp
            from scipy.sparse.linalg import eigsh
            Sh = sp.csr_matrix(((sc[dst] * sc[src]).numpy(), (dst, src)), shape=(n, n))
            ts = []
            for _ in range(a.reps if n < 50_000 else 1):                  # (tens of seconds at the large shape: once)
                t0 = time.perf_counter()
                w = eigsh(Sh, K, which="LA", tol=TOL, return_eigenvectors=True)[0]
                ts.append((time.perf_counter() - t0) * 1e3)
            row["scipy_eigsh_host_lanczos"] = series(ts)
            row["max_value_difference_vs_scipy"] = float(np.abs(np.sort(w)[::-1] - res.values.cpu().numpy()).max())
        # ---- the launches alone, on buffers of their own
        f64 = dict(dtype=torch.float64, device=dev)
        s = torch.empty(n, **f64)
        _lib.call("gae_spectral_scale", _ptr(indptr), n, 0.0, _ptr(s), _stream())
        V, AV, P = (torch.empty(n, B, **f64) for _ in range(3))
        _lib.call("gae_spectral_init", _ptr(V), n, B, 0, _stream())
        Gm, Hm, T = (torch.empty(B, B, **f64) for _ in range(3))
        values, resid = torch.empty(B, **f64), torch.empty(B, **f64)
        coef = torch.zeros(13, 3, **f64)
        coef[0, 0] = 1.0
        status = torch.zeros(8, dtype=torch.int64, device=dev)
        ws = torch.empty(lib.gae_spectral_workspace_bytes(n, nnz, B), dtype=torch.uint8, device=dev)

        def spmm(yin=V, yout=AV, ip=indptr, ix=indices, sv=s):
            _lib.call("gae_spectral_spmm", _ptr(ip), _ptr(ix), n, nnz, _ptr(sv), 0.0, _ptr(yin), None, _ptr(yout), B, _ptr(coef),
                      _ptr(status), _stream())

        def gram():
            _lib.call("gae_spectral_gram", _ptr(V), _ptr(AV), n, B, _ptr(Gm), _ptr(Hm), 0, _ptr(ws), ws.numel(), _stream())

        def solve():
            _lib.call("gae_spectral_solve", _ptr(Gm), _ptr(Hm), B, K, DEGREE, _ptr(T), _ptr(values), _ptr(coef), _ptr(status),
                      _ptr(ws), ws.numel(), _stream())
        spmm(); gram(); solve()
        Vr, AVr = V.clone(), AV.clone()
        eye = torch.eye(B, **f64)                                         # rotating by I keeps the operands finite over many launches

        def rotate():
            _lib.call("gae_spectral_rotate", _ptr(Vr), _ptr(AVr), n, B, K, _ptr(eye), _ptr(values), TOL, _ptr(resid), _ptr(status),
                      _ptr(ws), ws.numel(), _stream())
        t = {"spmm": bench.time_launches(spmm), "gram": bench.time_launches(gram),
             "solve": bench.time_launches(solve, iters=10, warmup=2), "rotate": bench.time_launches(rotate)}
        call_s = row["spectral"]["ms"] * 1e-3
        counts = {"spmm": res.n_spmm, "gram": res.n_iter, "solve": res.n_iter, "rotate": res.n_iter}
        row["kernels"] = {k: {"launch_us": v * 1e6, "launches_per_call": counts[k],
                              "share_of_call": v * counts[k] / call_s} for k, v in t.items()}
        row["host_and_other_share_of_call"] = 1.0 - sum(v["share_of_call"] for v in row["kernels"].values())
        # spmm: gather 8 b nnz + streams 8 b n in and out + indices and indptr and s
        sp_bytes = 8 * B * nnz + 2 * 8 * B * n + 4 * nnz + 4 * (n + 1) + 8 * n + 8 * nnz
        copy = bench.copy_bandwidth(sp_bytes, dev)
        ks = row["kernels"]["spmm"]
        ks.update(bytes=sp_bytes, GBs=sp_bytes / t["spmm"] / 1e9, copy_GBs=copy,
                  fraction_of_byte_bound=sp_bytes / t["spmm"] / 1e9 / copy)
        work = 2 * 8 * B * n + 4 * nnz + 4 * (n + 1) + 8 * n
        if work < (256 << 20):
            copies = bench.cold_copies(work)
            sets = [(V.clone(), torch.empty_like(AV), indptr.clone(), indices.clone(), s.clone()) for _ in range(copies)]
            t_cold = bench.time_rotation([(lambda q=q: spmm(*q)) for q in sets])
            ccold = bench.copy_bandwidth_cold(sp_bytes, dev)
            ks.update(launch_us_cold=t_cold * 1e6, copy_GBs_cold=ccold, fraction_of_byte_bound_cold=sp_bytes / t_cold / 1e9 / ccold,
                      cold_copies=copies)
            del sets
        for kname, nbytes, flops in (("gram", 2 * 8 * B * n, 2 * 2 * n * B * B), ("rotate", 4 * 8 * B * n, 2 * 2 * n * B * B)):
            copy = bench.copy_bandwidth(nbytes, dev)
            row["kernels"][kname].update(bytes=nbytes, GBs=nbytes / t[kname] / 1e9, copy_GBs=copy,
                                         fraction_of_copy_rate=nbytes / t[kname] / 1e9 / copy, flops=flops,
                                         fraction_of_fp64_matrix_peak=flops / t[kname] / FP64_MATRIX_PEAK)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
        del g, S, V, AV, P, Vr, AVr, ws
    result = {"what": "ops.spectral_embedding (K32: scale, init, then per outer iteration one product, the Gram pair, the "
                      "b x b solve in one block, the rotation with its residuals, one 64-byte host read, and a filter of 8 "
                      "products) on seeded random graphs; device-event timings of whole calls after warm-up, the series "
                      "alternating call by call in one process; ms = median.  kernels: the launches alone "
                      "(bench.time_launches, HIP-graph replay below 1 ms), share_of_call = launch time x launches per call "
                      "/ the call.  fraction_of_byte_bound: (gather 8 b nnz + 16 b n + indices, indptr, scales) / time over "
                      "the rate of a device copy moving the same bytes; _cold: rotating over disjoint operand copies.  "
                      "torch_same_schedule: torch.sparse.mm fp64, torch.linalg.cholesky / eigh, the same filter and "
                      "stopping rule, torch.randn start.  scipy_eigsh_host_lanczos: ARPACK on the host, a different algorithm",
              "reps": a.reps, "warmup": a.warmup, "rows": rows}
    text = json.dumps(result)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
