#!/usr/bin/env python3
"""Captured ZINC-shaped training steps (DeviceGraphDataset.synthetic_zinc, GAE 39 -> 32 -> 16, the library's Adam) with
the loss over the whole batch (scope "batch", the reference's loss) and per molecule (scope "graph",
gae_decoder_bce_graphs), timed in the same process: one CapturedInductiveStep per scope, replays alternating between
the two, each replay bracketed by device events on the current stream.  Prints one JSON object (and writes it with
--out).  For the kernel nodes of a step run it once more under `rocprofv3 --kernel-trace --stats` with --scopes graph.

    python tools/graph_scope_step.py --batches 128 4096 --steps 60 --out profiles/graph_scope_step.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 4096])
    ap.add_argument("--scopes", nargs="+", choices=["batch", "graph"], default=["batch", "graph"])
    ap.add_argument("--steps", type=int, default=60, help="timed replays per (batch size, scope)")
    ap.add_argument("--warmup", type=int, default=5, help="untimed replays per (batch size, scope) first")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import gae_dgl_amd as G
    from gae_dgl_amd.capture import CapturedInductiveStep
    from gae_dgl_amd.dataset import DeviceGraphDataset
    from gae_dgl_amd.optim import Adam
    dev = torch.device("cuda:0")
    result = {"what": "captured inductive step, ZINC-shaped synthetic set, GAE 39-32-16, Adam lr 1e-2; ms per step "
                      "from device events around each replay, scopes alternating", "steps": a.steps, "rows": []}
    for B in a.batches:
        n_batches = a.steps + a.warmup + 2
        ds = DeviceGraphDataset.synthetic_zinc(n_graphs=min(249455, B * n_batches), seed=0, device=dev)
        rng = np.random.default_rng(0)
        runners = {}
        for scope in a.scopes:
            torch.manual_seed(0)
            model = G.GAE(ds.n_feat, [32, 16]).to(dev)
            opt = Adam(model.parameters(), lr=1e-2)
            r = CapturedInductiveStep(model, opt, ds, B, loss_scope=scope)
            left = r.begin_epoch(rng.permutation(ds.ids))
            runners[scope] = [r, left, rng]
        times = {s: [] for s in a.scopes}
        losses = {s: [] for s in a.scopes}
        for it in range(a.warmup + a.steps):
            for scope in a.scopes:
                st = runners[scope]
                if st[1] == 0:
                    st[1] = st[0].begin_epoch(st[2].permutation(ds.ids))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                loss = st[0].step()
                e1.record()
                st[1] -= 1
                e1.synchronize()
                if it >= a.warmup:
                    times[scope].append(e0.elapsed_time(e1))
                    losses[scope].append(float(loss))
        for scope in a.scopes:
            t = np.asarray(times[scope])
            row = {"batch_graphs": B, "scope": scope, "median_ms": round(float(np.median(t)), 4),
                   "p10_ms": round(float(np.percentile(t, 10)), 4), "p90_ms": round(float(np.percentile(t, 90)), 4),
                   "mean_nodes": round(float(ds.sizes_host.mean()) * B, 1), "captures": runners[scope][0].captures,
                   "first_loss": losses[scope][0], "last_loss": losses[scope][-1]}
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
        del runners
        torch.cuda.synchronize()
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
