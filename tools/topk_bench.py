#!/usr/bin/env python3
"""Top-k link prediction (ops.decoder_topk, gae_decoder_topk) timed with device events after warm-up on random fp32
embeddings: Cora / Citeseer / Pubmed-sized Z with d = 16 and k in {1, 10, 64}, a ZINC-shaped 4096-molecule batch with
scope "graph", and n = 2e5 where no N x N matrix fits.  Beside each timing: the torch composite Z @ Z.T -> masked_fill
-> torch.topk where it fits (a baseline only; never on the product path), t_min = 2 n_pairs d / 157.3e12 and
frac_fp32 = t_min / t.  Prints one JSON object (and writes it with --out).  Kernel stats: run once more under
`rocprofv3 --kernel-trace --stats`.

    python tools/topk_bench.py --out profiles/r08_decoder_topk.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FP32 = 157.3e12


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(np.min(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="Pubmed only (k = --k)")
    ap.add_argument("--k", type=int, default=10, help="k of --quick")
    ap.add_argument("--no-composite", action="store_true", help="skip the torch baseline (counter runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import gae_dgl_amd as G
    from gae_dgl_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cases = [("pubmed", 19717, a.k)] if a.quick else \
        [(name, n, k) for name, n in (("cora", 2708), ("citeseer", 3327), ("pubmed", 19717)) for k in (1, 10, 64)]
    if not a.quick:
        cases += [("zinc4096_graph", None, 10), ("n200k", 200_000, 10)]
    rows = []
    for name, n, k in cases:
        d = 16
        g, scope = None, "batch"
        if name.startswith("zinc"):
            rng = np.random.default_rng(0)
            sizes = rng.integers(9, 39, 4096)
            gs = []
            for m in sizes:
                gr = G.DGLGraph(num_nodes=int(m))
                e = rng.integers(0, m, (2, 2 * int(m)))
                gr.add_edges(np.concatenate([e[0], e[1]]), np.concatenate([e[1], e[0]]))
                gs.append(gr.to(dev))
            g = G.batch(gs)
            n, scope = g.number_of_nodes(), "graph"
            pairs = float((sizes.astype(np.float64) ** 2).sum())
        else:
            pairs = float(n) * n
            gen = torch.Generator(device="cpu").manual_seed(1)
            src = torch.randint(0, n, (4 * n,), generator=gen)
            dst = torch.randint(0, n, (4 * n,), generator=gen)
            g = G.DGLGraph((torch.cat([src, dst]), torch.cat([dst, src])), num_nodes=n).to(dev)
        Z = torch.randn(n, d, device=dev)
        g.csr()
        med, mn = timed(lambda: ops.decoder_topk(Z, k, g, scope=scope), a.reps, a.warmup)
        row = {"case": name, "n": n, "d": d, "k": k, "scope": scope, "n_pairs": pairs, "ms": med, "ms_min": mn}
        t_min = 2 * pairs * d / PEAK_FP32
        row["t_min_ms"] = t_min * 1e3
        row["frac_fp32"] = t_min * 1e3 / med
        if scope == "batch" and n * n * 4 * 3 < 24e9 and not a.no_composite:
            indptr, indices = g.csr()
            rows_ = torch.repeat_interleave(torch.arange(n, device=dev), indptr[1:].long() - indptr[:-1].long())

            def composite():
                S = Z @ Z.T
                S.fill_diagonal_(float("-inf"))
                S[rows_, indices.long()] = float("-inf")
                return torch.topk(S, k, dim=1)
            cm, _ = timed(composite, max(3, a.reps // 4), 2)
            row["torch_composite_ms"] = cm
            row["speedup_vs_composite"] = cm / med
        else:
            row["torch_composite_ms"] = None
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    result = {"what": "ops.decoder_topk (gae_decoder_topk) on random fp32 Z, d = 16, known edges and self excluded; "
                      "ms = median of device-event timings after warm-up", "reps": a.reps, "rows": rows}
    text = json.dumps(result)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
