#!/usr/bin/env python3
"""The thresholded decoder (ops.decoder_threshold, gae_decoder_threshold_count / _fill) timed with device events after
warm-up on random fp32 embeddings, d = 16, self excluded, at n = 2 708, 19 717 and 200 000.  The threshold is the
0.999 quantile of a sample of logits, so about n^2 / 1000 pairs are listed; the count and the fill are also timed apart
(the profiler hook of the wrappers), and the call includes the one host sync that reads the total.
Where the N x N matrix fits (n <= 19 717) the route the library offered before is timed beside it, alternating call by
call: the reference-shaped dense logits (ops.decoder_dense, what GAE.forward ends in) followed by
``(logits >= tau).nonzero()``.  The spread of both series is recorded: the machines are shared.
Prints one JSON object (and writes it with --out).  No time or ratio is a pass condition.

    python tools/decode_bench.py --out profiles/r12_decoder_threshold.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="n = 19 717 only")
    ap.add_argument("--quantile", type=float, default=0.999, help="share of the logits below the threshold")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from gae_dgl_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cases = [("pubmed", 19717)] if a.quick else [("cora", 2708), ("pubmed", 19717), ("n200k", 200_000)]
    rows = []
    for name, n in cases:
        d = 16
        Z = torch.randn(n, d, device=dev)
        sample = Z[torch.randint(0, n, (2048,), device=dev)] @ Z[torch.randint(0, n, (2048,), device=dev)].T
        tau = float(torch.quantile(sample.reshape(-1), a.quantile))

        def decode():
            return ops.decoder_threshold(Z, tau, max_pairs=2 ** 31)
        for _ in range(a.warmup):
            links = decode()
        total = int(links.indptr[-1])
        dense = n <= 19717

        def composite():
            return (ops.decoder_dense(Z, None) >= tau).nonzero()
        if dense:
            for _ in range(2):
                dense_pairs = int(composite().shape[0])           # (the dense route keeps the diagonal)
        torch.cuda.synchronize()
        t_dec, t_dense = [], []
        for _ in range(a.reps):                                   # alternating: both series see the same neighbours
            t_dec.append(event_ms(decode))
            if dense:
                t_dense.append(event_ms(composite))
        ops.profiler = prof = ops.EventProfiler()
        try:
            for _ in range(max(3, a.reps // 4)):
                decode()
            parts = {k[0]: series([1e3 * s for s in v])["ms"] for k, v in prof.summary().items()}
        finally:
            ops.profiler = None
        row = {"case": name, "n": n, "d": d, "threshold": tau, "pairs": total, "output_bytes": 12 * total + 8 * (n + 1),
               "dense_matrix_bytes": 4 * n * n, "decoder_threshold": series(t_dec), "launch_ms": parts,
               "dense_then_nonzero": series(t_dense) if dense else None}
        if dense:
            row["dense_pairs"] = dense_pairs
            row["ratio_dense_over_threshold"] = row["dense_then_nonzero"]["ms"] / row["decoder_threshold"]["ms"]
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    result = {"what": "ops.decoder_threshold (gae_decoder_threshold_count / _fill, one host sync between them) on random "
                      "fp32 Z (d = 16), self excluded, threshold at the given quantile of the logits; beside it, where "
                      "the N x N matrix fits, ops.decoder_dense followed by (logits >= tau).nonzero(); device-event "
                      "timings after warm-up, the two series alternating call by call in one process; ms = median",
              "quantile": a.quantile, "reps": a.reps, "rows": rows}
    text = json.dumps(result)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
