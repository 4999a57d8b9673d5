#!/usr/bin/env python3
"""The sampled reconstruction loss (ops.decoder_bce_sampled_raw, gae_decoder_bce_sampled: forward + gradient in one
call) timed with device events, warm and MALL-cold (a 1 GiB buffer is written between calls), at m in {1, 4, 16, 64}
samples per row; beside it the fused exact loss where it runs, and the whole captured training step with the sampled
loss (m = 16).  Cases: Pubmed with planetoid-style hubs, the ZINC-4096 batch (one graph of 4096 molecules, batch
scope), and R-MAT s24 (2^24 nodes, 2^28 edges) as a real training step -- encoder, sampled loss, backward and Adam on
one GPU through parallel.ShardedTrainStep with world = 1.  bytes = 2 (E + n m) d 4 gathered + indices + the dZ write;
GB/s = bytes / warm time.  Prints one JSON object (and writes it with --out).

    python tools/sampled_loss_bench.py --out profiles/r09_sampled_loss.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

M_LIST = (1, 4, 16, 64)


def timed(fn, reps, warmup, flush=None):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        if flush is not None:
            flush.add_(1.0)                # evicts the 256 MB Infinity Cache (and the L2s) between calls
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), float(np.min(out))


def loss_bytes(n_local, E, m, d, n_ind):
    gathered = 2 * (E + n_local * m) * d * 4
    return gathered + 4 * n_ind + 2 * 4 * (n_local + 1) * 2 + n_local * d * 4


def loss_rows(name, Z, csr, csc, pw, E, a, flush, exact=None):
    from gae_dgl_amd import ops
    n, d = Z.shape
    draws = torch.zeros(1, dtype=torch.int64, device=Z.device)
    rows = []
    for m in M_LIST:
        fn = lambda: ops.decoder_bce_sampled_raw(Z, None, csr, csc, pw, m, seed=1, draws=draws)   # noqa: E731
        warm, warm_min = timed(fn, a.reps, a.warmup)
        cold, _ = timed(fn, max(3, a.reps // 2), 1, flush)
        nb = loss_bytes(n, E, m, d, 2 * E)
        rows.append({"case": name, "m": m, "n": n, "E": E, "d": d, "ms": warm, "ms_min": warm_min, "ms_cold": cold,
                     "bytes": nb, "GBps_warm": nb / warm / 1e6, "GBps_cold": nb / cold / 1e6})
        print(json.dumps(rows[-1]), file=sys.stderr)
    if exact is not None:
        fn = lambda: ops.decoder_bce_raw(Z, None, csr, csc, pw)                                    # noqa: E731
        warm, _ = timed(fn, a.reps, a.warmup)
        cold, _ = timed(fn, max(3, a.reps // 2), 1, flush)
        rows.append({"case": name, "m": "exact (decoder_bce)", "n": n, "E": E, "d": d, "ms": warm, "ms_cold": cold})
        print(json.dumps(rows[-1]), file=sys.stderr)
    return rows


def captured_step(g, X, m, a):
    import gae_dgl_amd as G
    from gae_dgl_amd.capture import CapturedTrainStep
    from gae_dgl_amd.optim import Adam
    torch.manual_seed(0)
    model = G.GAE(X.shape[1], [32, 16]).to(X.device)
    opt = Adam(model.parameters(), lr=1e-2)
    step = CapturedTrainStep(model, opt, g, X, loss_fn=lambda mm, gg: mm.reconstruction_loss(gg, samples=m), warmup=2)
    ms, ms_min = timed(step, a.reps, a.warmup)
    return {"ms": ms, "ms_min": ms_min, "loss_last": float(step())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-rmat", action="store_true", help="skip the R-MAT s24 case")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import gae_dgl_amd as G
    from gae_dgl_amd import ops, workloads as W
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    flush = torch.zeros(1 << 28, device=dev)
    result = {"what": "ops.decoder_bce_sampled_raw (gae_decoder_bce_sampled, loss + dZ); ms = median of device-event "
                      "timings, warm after warm-up, cold with a 1 GiB write between calls; step = captured training "
                      "step with the sampled loss at m = 16", "reps": a.reps, "loss": [], "step": []}
    # Pubmed, planetoid-style hubs
    n, src, dst, X = W.citation_graph("pubmed", degrees="planetoid")
    g = G.DGLGraph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=n).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    Z = torch.randn(n, 16, device=dev, generator=gen) * 0.3
    E = len(src)
    pw = (n * n - E) / E
    result["loss"] += loss_rows("pubmed_planetoid", Z, g.csr(), g.csc(), pw, E, a, flush, exact=True)
    Xd = ops.pad_rows(torch.from_numpy(X).to(dev))
    result["step"].append({"case": "pubmed_planetoid", "m": 16, **captured_step(g, Xd, 16, a)})
    print(json.dumps(result["step"][-1]), file=sys.stderr)
    # ZINC-4096: one batch of 4096 molecules, batch scope
    gptr, src, dst, X = W.zinc_like(4096, seed=0)
    n = int(gptr[-1])
    g = G.DGLGraph((torch.from_numpy(src), torch.from_numpy(dst)), num_nodes=n).to(dev)
    Z = torch.randn(n, 16, device=dev, generator=gen) * 0.3
    E = len(src)
    pw = (n * n - E) / E
    result["loss"] += loss_rows("zinc4096", Z, g.csr(), g.csc(), pw, E, a, flush, exact=True)
    result["step"].append({"case": "zinc4096", "m": 16,
                           **captured_step(g, ops.pad_rows(torch.from_numpy(X).to(dev)), 16, a)})
    print(json.dumps(result["step"][-1]), file=sys.stderr)
    del g, Z
    if not a.no_rmat:
        result.update(rmat(a, dev, flush))
    text = json.dumps(result)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


def rmat(a, dev, flush):
    """R-MAT s24 through parallel.ShardedTrainStep on a one-rank process group"""
    import torch.distributed as dist
    import gae_dgl_amd as G
    from gae_dgl_amd import workloads as W
    from gae_dgl_amd.optim import Adam
    from gae_dgl_amd.parallel import ShardedGraph, ShardedTrainStep
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29531")
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1)
    scale = 24
    n = 1 << scale
    src, dst = W.rmat_edges(scale, 16, seed=0, device=dev)
    E = int(src.numel())
    sg = ShardedGraph.from_edge_slice(n, src, dst, mode="allgather", device=dev)
    del src, dst
    torch.cuda.empty_cache()
    csr, csc = sg.csr_global("fwd"), sg.csr_global("bwd")
    gen = torch.Generator(device=dev).manual_seed(1234)
    Z = torch.randn(n, 16, device=dev, generator=gen) * 0.05
    pw = (float(n) * n - E) / E
    rows = loss_rows("rmat_s24", Z, csr, csc, pw, E, a, flush)
    del Z
    X = torch.rand(n, 32, device=dev, generator=gen)
    torch.manual_seed(0)
    model = G.GAE(32, [32, 16]).to(dev)
    opt = Adam(model.parameters(), lr=1e-2)
    step = ShardedTrainStep(model, opt, sg, X, transform_first=True, capture=True, warmup=2, loss_samples=16)
    ms, ms_min = timed(step, max(5, a.reps // 2), 2)
    losses = [float(step()) for _ in range(3)]
    out = {"case": "rmat_s24", "m": 16, "ms": ms, "ms_min": ms_min, "loss_last": losses,
           "what": "encoder (2 layers, 32 -> 32 -> 16, transform-first) + sampled loss + backward + Adam, captured, "
                   "ShardedTrainStep world = 1"}
    print(json.dumps(out), file=sys.stderr)
    return {"loss_rmat": rows, "step_rmat": out}


if __name__ == "__main__":
    main()
