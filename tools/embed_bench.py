#!/usr/bin/env python3
"""GAE.embed_graphs (ops.embed_graphs, gae_embed_graphs) timed with device events after warm-up on
DeviceGraphDataset.synthetic_zinc() at full size (249 455 molecules) and at 4 096 molecules, model 39 -> 32 -> 16: the
fused call against the route that existed before it, ``fused=False`` (batch -> encode -> readout_nodes in chunks of
4 096 graphs, and of 128 = the reference's default batch) -- the parent commit's code, untouched by K19 -- alternating
call by call in one process.  The spread of every series is recorded: the machines are shared.
Beside them: a device copy of the launch's algorithmic bytes (the measured copy rate gives the byte floor) and the flop
floor at the fp32 matrix / FMA peak, so the file says which of the two bounds the launch and at what fraction.  The
outputs of both routes are compared in the same run at the sizes timed.  Prints one JSON object (and writes it with
--out).  Kernel time: run once more under `rocprofv3 --kernel-trace --stats` with --fused-only.

    python tools/embed_bench.py --out profiles/r10_embed_graphs.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FP32_FLOPS = 157e12          # fp32 matrix / FMA peak of the MI355X
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


def algorithmic(ds, widths, n_graphs):
    """bytes and flop the fused launch needs, from the shapes: per atom its stored feature row, one row pointer and its
    column ids; per graph its node offset and 12 d bytes of output; 2 in out flop per atom and layer for the products
    plus 2 in per CSR entry and layer for the sums"""
    N, E = int(ds.n_nodes), int(ds.indices.numel())
    row_bytes = ds.feat.stride(0) * ds.feat.element_size()
    d = widths[-1]
    nbytes = N * (row_bytes + 4) + E * 4 + n_graphs * (8 + 12 * d)
    ins = [ds.n_feat] + widths[:-1]
    flop = sum(2 * N * i * o + 2 * E * i for i, o in zip(ins, widths))
    return {"N": N, "E": E, "G": n_graphs, "bytes": int(nbytes), "flop": int(flop), "feature_row_bytes": int(row_bytes)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reps128", type=int, default=3, help="calls of the batch-128 route at full size (about a second each)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="4 096 molecules only")
    ap.add_argument("--fused-only", action="store_true", help="time the fused call alone (kernel-trace runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import gae_dgl_amd as G
    from gae_dgl_amd.dataset import DeviceGraphDataset
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = G.GAE(39, HIDDEN).to(dev)
    rows = []
    for name, n_graphs in ([("zinc_4096", 4096)] if a.quick else [("zinc_4096", 4096), ("zinc_full", 249455)]):
        ds = DeviceGraphDataset.synthetic_zinc(n_graphs, seed=0, device=dev)
        alg = algorithmic(ds, HIDDEN, n_graphs)

        def fused():
            return model.embed_graphs(ds, fused=True)

        def chunked(bs):
            return model.embed_graphs(ds, fused=False, batch_size=bs)
        buf = torch.empty(alg["bytes"], dtype=torch.uint8, device=dev)
        dst = torch.empty_like(buf)

        def copy():
            dst.copy_(buf)
        row = {"case": name, "model": [39] + HIDDEN, "algorithmic": alg}
        for _ in range(a.warmup):
            fused(); copy()
            if not a.fused_only:
                chunked(4096)
        if not a.fused_only:
            chunked(128)
        torch.cuda.synchronize()
        t_f, t_c, t_4096, t_128 = [], [], [], []
        n128 = a.reps if n_graphs <= 4096 else a.reps128
        for r in range(a.reps):                                   # alternating: every series sees the same neighbours
            t_f.append(event_ms(fused))
            t_c.append(event_ms(copy))
            if not a.fused_only:
                t_4096.append(event_ms(lambda: chunked(4096)))
                if r < n128:
                    t_128.append(event_ms(lambda: chunked(128)))
        row["fused"] = series(t_f)
        row["copy_of_algorithmic_bytes"] = series(t_c)
        copy_rate = 2 * alg["bytes"] / (row["copy_of_algorithmic_bytes"]["ms"] * 1e-3)       # read + write
        floor_bytes_ms = alg["bytes"] / copy_rate * 1e3
        floor_flop_ms = alg["flop"] / PEAK_FP32_FLOPS * 1e3
        row["floors"] = {"copy_rate_GBps": copy_rate / 1e9, "bytes_floor_ms": floor_bytes_ms, "flop_floor_ms": floor_flop_ms,
                         "bound_by": "flop" if floor_flop_ms > floor_bytes_ms else "bytes",
                         "fused_call_fraction_of_bytes_floor": floor_bytes_ms / row["fused"]["ms"],
                         "fused_call_fraction_of_flop_floor": floor_flop_ms / row["fused"]["ms"]}
        if not a.fused_only:
            row["chunked_batch4096"] = series(t_4096)
            row["chunked_batch128"] = series(t_128)
            row["speedup_over_batch4096"] = row["chunked_batch4096"]["ms"] / row["fused"]["ms"]
            row["speedup_over_batch128"] = row["chunked_batch128"]["ms"] / row["fused"]["ms"]
            row["separated_by_more_than_the_spread"] = bool(row["chunked_batch4096"]["ms_p10"] > row["fused"]["ms_p90"])
            f, c = fused().double(), chunked(4096).double()
            scale = max(1.0, float(c.abs().max()))
            row["max_abs_diff_over_scale_fused_vs_batch4096"] = float((f - c).abs().max()) / scale
            row["fused_bitwise_repeatable"] = bool(torch.equal(fused(), fused()))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
        del ds, buf, dst
    result = {"what": "GAE.embed_graphs on DeviceGraphDataset.synthetic_zinc (uint8 features), model 39 -> 32 -> 16: the "
                      "fused launch (gae_embed_graphs) against fused=False (batch -> encode -> readout_nodes in chunks); "
                      "device-event timings of whole calls after warm-up, the series alternating call by call in one "
                      "process; ms = median",
              "yardstick": "fused=False runs the routes of the parent commit: dataset.batch, GAE.encode and "
                           "readout_nodes are untouched by K19",
              "peak_fp32_flops": PEAK_FP32_FLOPS, "reps": a.reps, "rows": rows}
    text = json.dumps(result)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
