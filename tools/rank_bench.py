#!/usr/bin/env python3
"""Filtered link ranking (ops.decoder_rank, gae_decoder_rank) timed with device events after warm-up on random fp32
embeddings, d = 16, self and the edges of a random 5-regular graph excluded: m = n queries (src = arange(n), random
dst) at n = 2 708, 19 717 and 200 000, and the evaluation-shaped case n = 200 000 with m = 2e5 random sources.
Beside each, in the same process and alternating with it call by call, the yardstick: ops.decoder_topk(Z, 10, g) on the
same Z and graph (gae_decoder_topk sweeps the same n x n products with the same MFMA chain, csrc/decoder_pairs.h).  The
spread of both series is recorded: the machines are shared.
Where it fits (n <= 19 717) the torch route (Z[src] @ Z.T, compare, sum) is timed for scale only; it is never on the
product path.  Prints one JSON object (and writes it with --out).  Kernel stats: run once more under
`rocprofv3 --kernel-trace --stats`.

    python tools/rank_bench.py --out profiles/r09_decoder_rank.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BAR = 1.5          # decoder_rank at m = n may take this many times decoder_topk(k = 10), at n = 19 717 and 200 000


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
    ap.add_argument("--no-composite", action="store_true", help="skip the torch route (kernel-trace runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import gae_dgl_amd as G
    from gae_dgl_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cases = [("pubmed_m=n", 19717, None)] if a.quick else \
        [("cora_m=n", 2708, None), ("pubmed_m=n", 19717, None), ("n200k_m=n", 200_000, None),
         ("n200k_eval_m=2e5", 200_000, 200_000)]
    rows = []
    for name, n, m_random in cases:
        d, deg = 16, 5
        gen = torch.Generator(device="cpu").manual_seed(1)
        g = G.DGLGraph((torch.randint(0, n, (deg * n,), generator=gen), torch.arange(n).repeat_interleave(deg)),
                       num_nodes=n).to(dev)                       # every node has 5 in-edges: CSR rows of 5
        g.csr()
        Z = torch.randn(n, d, device=dev)
        if m_random is None:
            src = torch.arange(n)
        else:
            src = torch.randint(0, n, (m_random,), generator=gen)
        m = src.numel()
        pairs = torch.stack([src, torch.randint(0, n, (m,), generator=gen)]).to(dev)

        def rank():
            return ops.decoder_rank(Z, pairs, g)

        def topk():
            return ops.decoder_topk(Z, 10, g)
        for _ in range(a.warmup):
            rank(); topk()
        torch.cuda.synchronize()
        t_rank, t_topk = [], []
        for _ in range(a.reps):                                   # alternating: both series see the same neighbours
            t_rank.append(event_ms(rank))
            t_topk.append(event_ms(topk))
        row = {"case": name, "n": n, "m": m, "d": d, "in_degree": deg, "decoder_rank": series(t_rank),
               "decoder_topk_k10": series(t_topk)}
        row["ratio_rank_over_topk"] = row["decoder_rank"]["ms"] / row["decoder_topk_k10"]["ms"]
        if m_random is None and n in (19717, 200_000):
            row["bar"] = BAR
            row["within_bar"] = bool(row["ratio_rank_over_topk"] <= BAR)
        if n <= 19717 and not a.no_composite:
            indptr, indices = g.csr()
            rows_ = torch.repeat_interleave(torch.arange(n, device=dev), indptr[1:].long() - indptr[:-1].long())
            q = torch.arange(m, device=dev)

            def composite():
                S = Z[pairs[0]] @ Z.T
                t = S[q, pairs[1]].clone()
                S[q, pairs[0]] = float("-inf")                    # self (m = n, src = arange(n): row q is node q)
                S[rows_, indices.long()] = float("-inf")
                S[q, pairs[1]] = float("-inf")
                return (S > t[:, None]).sum(1), (S == t[:, None]).sum(1)
            for _ in range(2):
                composite()
            torch.cuda.synchronize()
            row["torch_route_ms"] = series([event_ms(composite) for _ in range(max(3, a.reps // 4))])["ms"]
        else:
            row["torch_route_ms"] = None
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    result = {"what": "ops.decoder_rank (gae_decoder_rank) against ops.decoder_topk(k = 10) on the same random fp32 Z "
                      "(d = 16) and 5-regular graph, self and known edges excluded; device-event timings after "
                      "warm-up, the two series alternating call by call in one process; ms = median",
              "yardstick": "gae_decoder_topk of this library, on the same products (csrc/decoder_pairs.h)",
              "reps": a.reps, "rows": rows}
    text = json.dumps(result)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
