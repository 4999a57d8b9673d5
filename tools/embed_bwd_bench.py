#!/usr/bin/env python3
"""Forward + backward of the molecule feature through the fused kernel pair (K19 gae_embed_graphs + K21
gae_embed_graphs_bwd behind GAE.embed_graphs(grad=True, fused=True)) timed with device events after warm-up on
DeviceGraphDataset.synthetic_zinc(): the whole resident set (249 455 molecules) in one call, and steps of 4 096 and of
128 molecules taken as subset() views of the same resident set; model 39 -> 32 -> 16, loss = sum(features * d_out).
Baseline: the route that can be written on the parent commit with no new kernel -- batch -> encode -> a torch segment
readout (index_add / scatter_reduce amax) -> backward, in chunks of 4 096 graphs (a step of 128 is one chunk of 128).
Beside it the chunked route of this commit (fused=False: the same, with ops.segment_readout and its own backward
kernel).  The series alternate call by call in one process and the spread of each is recorded: the machines are
shared.  The gradients of the routes are compared in the same run.  Prints one JSON object (and writes it with --out).
Kernel time: run once more under `rocprofv3 --kernel-trace --stats` with --fused-only.

    python tools/embed_bwd_bench.py --out profiles/r11_embed_bwd.json
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


def torch_readout(z, gp):
    """[mean | sum | max] per member graph with torch ops alone (what the parent commit allows under autograd)"""
    sizes = gp[1:] - gp[:-1]
    G, (N, d) = sizes.numel(), z.shape
    gid = torch.repeat_interleave(torch.arange(G, device=z.device), sizes, output_size=N)
    s = torch.zeros(G, d, dtype=z.dtype, device=z.device).index_add(0, gid, z)
    mean = s / sizes.clamp(min=1).to(z.dtype).unsqueeze(1)
    mx = torch.full((G, d), -float("inf"), dtype=z.dtype, device=z.device)
    mx = mx.scatter_reduce(0, gid.unsqueeze(1).expand(N, d), z, "amax", include_self=True)
    return torch.cat([mean, s, mx], 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="a resident set of 8 192 molecules")
    ap.add_argument("--fused-only", action="store_true", help="time the fused pair alone (kernel-trace runs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import gae_dgl_amd as G
    from gae_dgl_amd.dataset import DeviceGraphDataset
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = G.GAE(39, HIDDEN).to(dev)
    params = list(model.parameters())
    n_set = 8192 if a.quick else 249455
    ds = DeviceGraphDataset.synthetic_zinc(n_set, seed=0, device=dev)
    rng = np.random.default_rng(0)
    d_all = torch.randn(n_set, 3 * HIDDEN[-1], device=dev)
    rows = []
    for name, n in (("step_128", 128), ("step_4096", 4096), ("whole_set", n_set)):
        ids = np.arange(n_set) if n == n_set else np.sort(rng.permutation(n_set)[:n])
        view = ds if n == n_set else ds.subset(ids)
        d_out = d_all[torch.from_numpy(ids).to(dev)]

        def clear():
            for p in params:
                p.grad = None

        def fused():
            clear()
            (model.embed_graphs(view, fused=True, grad=True) * d_out).sum().backward()

        def chunked():                                # this commit's chunked route
            clear()
            (model.embed_graphs(view, fused=False, batch_size=4096, grad=True) * d_out).sum().backward()

        def baseline():                               # the parent commit's means: torch ops for the readout
            clear()
            for lo in range(0, n, 4096):
                bg = ds.batch(ids[lo:lo + 4096])
                f = torch_readout(model.encode(bg), bg.graph_ptr())
                (f * d_out[lo:lo + 4096]).sum().backward()

        def grads(fn):
            fn()
            return [p.grad.detach().double().clone() for p in params]
        row = {"case": name, "molecules": n, "resident_set": n_set, "model": [39] + HIDDEN}
        for _ in range(a.warmup):
            fused()
            if not a.fused_only:
                chunked(); baseline()
        torch.cuda.synchronize()
        t_f, t_c, t_b = [], [], []
        for _ in range(a.reps):                       # alternating: every series sees the same neighbours
            t_f.append(event_ms(fused))
            if not a.fused_only:
                t_c.append(event_ms(chunked))
                t_b.append(event_ms(baseline))
        row["fused_pair"] = series(t_f)
        if not a.fused_only:
            row["chunked_readout_kernel"] = series(t_c)
            row["baseline_torch_readout"] = series(t_b)
            row["speedup_over_baseline"] = row["baseline_torch_readout"]["ms"] / row["fused_pair"]["ms"]
            row["speedup_over_chunked"] = row["chunked_readout_kernel"]["ms"] / row["fused_pair"]["ms"]
            row["separated_by_more_than_the_spread"] = bool(row["baseline_torch_readout"]["ms_p10"] > row["fused_pair"]["ms_p90"])
            gf, gb, gc = grads(fused), grads(baseline), grads(chunked)
            rel = lambda x, y: max(float((u - v).abs().max() / v.abs().max().clamp(min=1.0)) for u, v in zip(x, y))   # noqa: E731
            row["max_rel_diff_fused_vs_baseline"] = rel(gf, gb)
            row["max_rel_diff_chunked_vs_baseline"] = rel(gc, gb)
            row["fused_bitwise_repeatable"] = bool(all(torch.equal(u, v) for u, v in zip(gf, grads(fused))))
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    result = {"what": "forward + backward of the molecule feature, GAE.embed_graphs(grad=True) on "
                      "DeviceGraphDataset.synthetic_zinc (uint8 features), model 39 -> 32 -> 16, loss = sum(features * "
                      "d_out): the fused kernel pair (gae_embed_graphs + gae_embed_graphs_bwd) against batch -> encode -> "
                      "torch segment readout -> backward in chunks of 4 096 (baseline) and against fused=False of this "
                      "commit (the readout and its backward as kernels); device-event timings of whole calls after "
                      "warm-up, the series alternating call by call in one process; ms = median",
              "yardstick": "the baseline uses dataset.batch, GAE.encode and torch ops only: it runs unchanged on the "
                           "parent commit",
              "reps": a.reps, "rows": rows}
    text = json.dumps(result)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
