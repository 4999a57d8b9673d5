#!/usr/bin/env python3
"""Exact k-nearest-neighbour search on the device (ops.knn: gae_knn, K24) timed with device events after warm-up on seeded
normal data at four shapes: the self-search of Pubmed's embedding (m = n = 19 717, d = 16, k = 10), the kNN graph of
the molecule features of embed_graphs (m = n = 249 455, d = 48, k = 10), 4096 queries against that set with k = 64,
and an inner-product self-search at n = 2 * 10^5, d = 16.  Beside it, alternating call by call, the route a user had
before: ``torch.cdist`` (or the matrix product) -> ``topk`` over chunks of queries sized so that the chunk x n matrix
stays under 1 GiB; for the inner-product row also ``ops.decoder_topk(exclude_edges=False)`` (K16) on the same Z, which
does the same products and selection.  ``--probe`` adds what tells product, selection and the X stream apart at the
molecule shape: the same 32 768 queries with k = 1, 10 and 64, with d = 16 and 48, and against a database cut to
the size of one L2.  The spread of every series is recorded: the machines are shared.
Prints one JSON object (and writes it with --out).  No time or ratio is a pass condition.

    python tools/knn_bench.py --probe --out profiles/r14_knn.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [("pubmed_z", 19717, 19717, 16, 10, "l2"), ("zinc_features", 249_455, 249_455, 48, 10, "l2"),
         ("zinc_queries", 4096, 249_455, 48, 64, "l2"), ("n200k_dot", 200_000, 200_000, 16, 10, "dot")]
FP32_MFMA_PEAK = 157.3e12         # v_mfma_f32_32x32x2_f32: 256 FLOP / clk / CU, 256 CUs, 2.4 GHz
GIB = 1 << 30


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


def torch_knn(Q, X, k, metric, same):
    """cdist (l2) or the product (dot) and topk over query chunks whose chunk x n matrix stays under 1 GiB"""
    n = X.shape[0]
    chunk = max(1, GIB // (4 * n))
    idx, val = [], []
    for r0 in range(0, Q.shape[0], chunk):
        q = Q[r0:r0 + chunk]
        s = torch.cdist(q, X) if metric == "l2" else q @ X.t()
        if same:
            rows = torch.arange(q.shape[0], device=Q.device)
            s[rows, rows + r0] = float("inf") if metric == "l2" else float("-inf")
        v, i = torch.topk(s, k, dim=1, largest=metric != "l2")
        idx.append(i); val.append(v)
    return torch.cat(idx), torch.cat(val)


def normal(n, d, seed, dev):
    return torch.randn(n, d, generator=torch.Generator(device="cpu").manual_seed(seed)).to(dev)


def peak_fraction(m, n, d, ms):
    return 2.0 * m * n * d / (ms * 1e-3) / FP32_MFMA_PEAK


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--big_reps", type=int, default=5, help="repetitions where m n exceeds 10^10")
    ap.add_argument("--case", choices=[c[0] for c in CASES], default=None, help="one shape only (kernel traces)")
    ap.add_argument("--no_torch", action="store_true", help="skip the torch route")
    ap.add_argument("--probe", action="store_true", help="also the product / selection / X-stream probe")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from gae_dgl_amd import ops
    dev = torch.device("cuda:0")
    rows = []
    for name, m, n, d, k, metric in [c for c in CASES if a.case in (None, c[0])]:
        X = normal(n, d, 0, dev)
        same = m == n
        Q = X if same else normal(m, d, 1, dev)
        reps = a.reps if m * n <= 10 ** 10 else min(a.reps, a.big_reps)

        def native():
            return ops.knn(Q, None if same else X, k=k, metric=metric)

        routes = {"knn": native}
        if not a.no_torch:
            routes["torch_chunked_topk"] = lambda: torch_knn(Q, X, k, metric, same)
        if metric == "dot" and same:
            routes["decoder_topk"] = lambda: ops.decoder_topk(Q, k, exclude_edges=False)
        times = {r: [] for r in routes}
        out = {}
        for rep in range(a.warmup + reps):                            # alternating: every series sees the same neighbours
            for r, fn in routes.items():
                if r == "torch_chunked_topk" and rep >= a.warmup + min(reps, 3) and m * n > 10 ** 10:
                    continue                                          # seconds per call at the largest shapes
                t = event_ms(lambda: out.__setitem__(r, fn()))
                if rep >= a.warmup:
                    times[r].append(t)
        row = {"case": name, "m": m, "n": n, "d": d, "k": k, "metric": metric, "distance_matrix_bytes": 4 * m * n}
        for r in routes:
            row[r] = series(times[r])
        row["knn_fp32_matrix_peak_fraction"] = peak_fraction(m, n, d, row["knn"]["ms"])
        if "torch_chunked_topk" in routes:
            row["ratio_torch_over_knn"] = row["torch_chunked_topk"]["ms"] / row["knn"]["ms"]
            ti = out["torch_chunked_topk"][0]
            row["index_equal_fraction_vs_torch"] = float((out["knn"].index.long() == ti).double().mean())
        if "decoder_topk" in routes:
            row["ratio_decoder_topk_over_knn"] = row["decoder_topk"]["ms"] / row["knn"]["ms"]
            row["decoder_topk_fp32_matrix_peak_fraction"] = peak_fraction(m, n, d, row["decoder_topk"]["ms"])
            row["bits_equal_to_decoder_topk"] = bool(torch.equal(out["knn"].index.long(), out["decoder_topk"][1])
                                                     and torch.equal(out["knn"].value, out["decoder_topk"][0]))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
        del X, Q, out
    probe = []
    if a.probe:
        # one variable at a time from (m = 32 768, n = 249 455, d = 48, k = 10, l2): k moves the selection only; d moves
        # the product and the stream together; n = 16 384 (3 MB of X: inside one L2) with m raised to about the same
        # number of pairs takes the stream out.  The time PER PAIR is what is compared
        for m, n, d, k in [(32768, 249_455, 48, 1), (32768, 249_455, 48, 10), (32768, 249_455, 48, 64),
                           (32768, 249_455, 16, 10), (32768, 249_455, 64, 10), (499_712, 16384, 48, 10)]:
            X, Q = normal(n, d, 2, dev), normal(m, d, 3, dev)
            ts = [event_ms(lambda: ops.knn(Q, X, k=k)) for _ in range(a.warmup + a.reps)][a.warmup:]
            s = series(ts)
            probe.append({"m": m, "n": n, "d": d, "k": k, **s, "ns_per_1000_pairs": s["ms"] * 1e6 / (m * n / 1000.0),
                          "fp32_matrix_peak_fraction": peak_fraction(m, n, d, s["ms"])})
            print(json.dumps(probe[-1]), file=sys.stderr)
            del X, Q
    result = {"what": "ops.knn (gae_knn: h, sweep, merge of the splits, direct distances; its allocations included) "
                      "against torch.cdist / matmul -> topk over query chunks under 1 GiB and, for the dot row, "
                      "ops.decoder_topk(exclude_edges=False) on the same Z; seeded standard normal data; device-event "
                      "timings of whole calls after warm-up, the series alternating call by call in one process; "
                      "ms = median; peak fraction = 2 m n d / time / 157.3 TFLOP/s (fp32 MFMA); the torch route is "
                      "timed at most 3 times where m n > 10^10",
              "reps": a.reps, "warmup": a.warmup, "rows": rows, "probe": probe}
    text = json.dumps(result)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
