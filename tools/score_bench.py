#!/usr/bin/env python3
"""GAE.score_graphs (ops.score_graphs, gae_score_graphs, K20) timed with device events after warm-up on
DeviceGraphDataset.synthetic_zinc() at full size (249 455 molecules) and at 4 096 molecules, model 39 -> 32 -> 16:
the fused call, GAE.embed_graphs (K19: the same encoder with the readout tail -- the encoder's share) and the chunked
route ``fused=False`` (batch -> encode in chunks of 4 096 graphs, Z scored by the kernel's no-layer mode), alternating
call by call in one process.  The spread of every series is recorded: the machines are shared.  The two routes' results
are compared in the same run.  Prints one JSON object (and writes it with --out).  Kernel time: run once more under
`rocprofv3 --kernel-trace --stats` with --fused-only.

    python tools/score_bench.py --out profiles/r11_score_graphs.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HIDDEN = [32, 16]


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
            "ms_p10": float(np.percentile(xs, 10)), "ms_p90": float(np.percentile(xs, 90)), "calls": int(xs.size)}


def work(scores, sizes):
    """what the tail does, from the shapes: logits n^2 d, and per positive one compare pair per unordered pair of its
    graph plus one per positive"""
    n = torch.as_tensor(sizes, dtype=torch.float64)
    p = scores.n_pos.double().cpu()
    return {"logit_fma": float((n * n).sum()) * HIDDEN[-1], "compares": float((p * (n * (n - 1) / 2 + p)).sum()) * 2,
            "positives": float(p.sum()), "pairs": float((n * (n - 1)).sum())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="4 096 molecules only")
    ap.add_argument("--fused-only", action="store_true", help="time the two fused calls alone (kernel-trace runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import gae_dgl_amd as G
    from gae_dgl_amd import metrics
    from gae_dgl_amd.dataset import DeviceGraphDataset
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = G.GAE(39, HIDDEN).to(dev)
    rows = []
    for name, n_graphs in ([("zinc_4096", 4096)] if a.quick else [("zinc_4096", 4096), ("zinc_full", 249455)]):
        ds = DeviceGraphDataset.synthetic_zinc(n_graphs, seed=0, device=dev)

        def fused():
            return model.score_graphs(ds, fused=True)

        def embed():
            return model.embed_graphs(ds, fused=True)

        def chunked():
            return model.score_graphs(ds, fused=False, batch_size=4096)
        row = {"case": name, "model": [39] + HIDDEN, "N": int(ds.n_nodes), "E": int(ds.indices.numel()), "G": n_graphs}
        for _ in range(a.warmup):
            fused(); embed()
            if not a.fused_only:
                chunked()
        torch.cuda.synchronize()
        t_f, t_e, t_c = [], [], []
        for _ in range(a.reps):                                   # alternating: every series sees the same neighbours
            t_f.append(event_ms(fused))
            t_e.append(event_ms(embed))
            if not a.fused_only:
                t_c.append(event_ms(chunked))
        row["score_graphs_fused"] = series(t_f)
        row["embed_graphs_fused"] = series(t_e)
        row["score_over_embed"] = row["score_graphs_fused"]["ms"] / row["embed_graphs_fused"]["ms"]
        f = fused()
        row["work"] = work(f, ds.sizes_host[np.asarray(ds.ids)])
        row["summary"] = metrics.graph_score_summary(f)
        row["fused_bitwise_repeatable"] = bool(all(torch.equal(torch.nan_to_num(x, nan=-7.0) if x.is_floating_point() else x,
                                                               torch.nan_to_num(y, nan=-7.0) if y.is_floating_point() else y)
                                                   for x, y in zip(f, fused())))
        if not a.fused_only:
            row["chunked_batch4096_no_layer_mode"] = series(t_c)
            row["speedup_over_chunked"] = row["chunked_batch4096_no_layer_mode"]["ms"] / row["score_graphs_fused"]["ms"]
            row["separated_by_more_than_the_spread"] = bool(row["chunked_batch4096_no_layer_mode"]["ms_p10"] >
                                                            row["score_graphs_fused"]["ms_p90"])
            c = chunked()
            row["counts_differ_fused_vs_chunked"] = int((f.wins != c.wins).sum())     # Z differs in the last bits
            row["max_abs_auc_diff_fused_vs_chunked"] = float(torch.nan_to_num(f.auc - c.auc).abs().max())
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
        del ds
    result = {"what": "GAE.score_graphs on DeviceGraphDataset.synthetic_zinc (uint8 features), model 39 -> 32 -> 16: the "
                      "fused launch (gae_score_graphs) beside GAE.embed_graphs (gae_embed_graphs, the encoder's share) "
                      "and the chunked route (batch -> encode, Z scored by the no-layer mode); device-event timings of "
                      "whole calls after warm-up, the series alternating call by call in one process; ms = median",
              "reps": a.reps, "rows": rows}
    text = json.dumps(result)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
