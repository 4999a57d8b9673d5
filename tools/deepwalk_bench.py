#!/usr/bin/env python3
"""The DeepWalk baseline (ops.random_walks: gae_random_walks, K37; ops.sgns_train: gae_sgns_accumulate / gae_sgns_update, K38)
timed with device events after a warm-up on the Cora-sized, Pubmed-sized and 2 10^5-node graphs of tools/neighbour_bench.py, at
the defaults of ops.deepwalk (dim 64, 10 walks of 40 per node, window 5, K = 5, M = 16, batches of 256 walks):
  walks       the walk launch alone on a preallocated table, and the whole ops.random_walks call;
  epoch       one epoch of ops.sgns_train (the walk order, two launches per batch, one status read);
  accumulate  the gradient launch of one full batch alone, the tables as the epoch left them;
  update      the Adagrad sweep alone, on accumulators that batch filled (refilled outside the timing).
Beside them the same schedule written in torch on the same device: gathered rows, torch.bmm for the logits and the three
gradient products, index_add_ into dense fp32 gradient tables, a dense Adagrad sweep -- fp32 atomics and another stream of
negatives (torch.searchsorted on the same noise table), so its bits differ run to run; it is there for the time.
Recorded with every time: the bytes the update sweep must move at the least (8 bytes of accumulator per element of both
tables, 16 more per touched element) and the share of the measured HBM copy rate (6.29 TB/s) that makes of the sweep's time; the
fp32 matrix-instruction work of a batch (2 LP (LP + M) dP + 2 (LP + M) LP dP + 2 LP (LP + M) dP flop per walk, padded sizes) and
the time it would take at the fp32 matrix peak (157.3 TF).  The spread of every series is recorded: the machines are shared.
Prints one JSON object (and writes it with --out).  No time or ratio is a pass condition.

    python tools/deepwalk_bench.py --out profiles/r27_deepwalk.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from neighbour_bench import SHAPES, event_ms, planetoid_like, series  # noqa: E402

HBM_COPY_BYTES_PER_S, FP32_MATRIX_FLOPS = 6.29e12, 157.3e12
DIM, R, L, WINDOW, K, M, BATCH, LR, EPS = 64, 10, 40, 5, 5, 16, 256, 0.05, 1e-8


def torch_epoch(walks, cum, W, C, HW, HC, order, gen):
    """the same schedule in torch: one pass over the walks in `order`, batches of BATCH"""
    dev = W.device
    n, d = W.shape
    total = float(cum[-1])
    p = torch.arange(L, device=dev)
    dist = (p[:, None] - p[None, :]).abs()
    near = (dist > 0) & (dist <= WINDOW)
    GW, GC = torch.zeros_like(W), torch.zeros_like(C)
    for first in range(0, order.numel(), BATCH):
        ids = walks[order[first:first + BATCH].long()].long()
        B = ids.shape[0]
        valid = ids >= 0
        safe = ids.clamp(min=0)
        u = torch.rand(B, M, device=dev, generator=gen, dtype=torch.float64) * total
        neg = (torch.searchsorted(cum, u.to(torch.int64), right=True) - 1).clamp(0, n - 1)
        Ww = W[safe] * valid[..., None]
        Cc = torch.cat([C[safe] * valid[..., None], C[neg]], 1)
        SN = torch.bmm(Ww, Cc.transpose(1, 2))
        pos = near[None] & valid[:, :, None] & valid[:, None, :]
        coef = pos.sum(2).float() * (K / M)
        Gp = torch.sigmoid(-SN[:, :, :L]) * pos
        Gn = -(coef[:, :, None] * torch.sigmoid(SN[:, :, L:])) * ((neg[:, None, :] != ids[:, :, None]) & valid[:, :, None])
        Gm = torch.cat([Gp, Gn], 2)
        dW = torch.bmm(Gm, Cc) * valid[..., None]
        dC = torch.bmm(Gm.transpose(1, 2), Ww)
        GW.index_add_(0, safe.reshape(-1), dW.reshape(-1, d))
        GC.index_add_(0, torch.cat([safe, neg], 1).reshape(-1), (dC * torch.cat([valid, torch.ones_like(neg, dtype=torch.bool)],
                                                                                1)[..., None]).reshape(-1, d))
        for X, H, Gd in ((W, HW, GW), (C, HC, GC)):
            H.addcmul_(Gd, Gd)
            X.addcdiv_(Gd, H.sqrt() + EPS, value=LR)
            Gd.zero_()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", nargs="+", default=[s[0] for s in SHAPES])
    ap.add_argument("--no_torch", action="store_true", help="skip the torch route")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import gae_dgl_amd as G
    from gae_dgl_amd import _lib, ops
    from gae_dgl_amd.ops import _ptr, _stream
    dev = torch.device("cuda:0")

    def timed(routes, before=None):
        times = {r: [] for r in routes}
        for rep in range(a.warmup + a.reps):                               # alternating: every series sees the same neighbours
            for r, fn in routes.items():
                if before is not None:
                    before(r)
                t = event_ms(fn)
                if rep >= a.warmup:
                    times[r].append(t)
        return {r: series(times[r]) for r in routes}

    rows = []
    for name, n, edges, hubs in SHAPES:
        if name not in a.shapes:
            continue
        src, dst = planetoid_like(n, edges, hubs, seed=0)
        g = G.DGLGraph((src, dst), num_nodes=n).to(dev)
        indptr, indices = g.csr()
        wide = indptr.long().contiguous()
        n_walks = n * R
        table = torch.empty(n_walks, L, dtype=torch.int32, device=dev)
        status = torch.zeros(_lib.DEEPWALK_STATUS_WORDS, dtype=torch.int64, device=dev)

        def walks_kernel():
            _lib.call("gae_random_walks", _ptr(wide), _ptr(indices), n, indices.numel(), None, n, R, L, 0, _ptr(table), _ptr(status),
                      _stream())
        row = {"case": name, "n": n, "nnz": indices.numel(), "n_walks": n_walks, "dim": DIM, "walk_length": L, "window": WINDOW,
               "negatives": K, "shared_negatives": M, "batch_walks": BATCH, "n_batches": -(-n_walks // BATCH)}
        row.update(timed({"walks_kernel": walks_kernel,
                          "walks_call": lambda: ops.random_walks(g, walks_per_node=R, walk_length=L, seed=0)}))
        walks = ops.random_walks(g, walks_per_node=R, walk_length=L, seed=0)
        row["walk_steps_per_us"] = float((walks[:, 1:] >= 0).sum()) / (row["walks_kernel"]["ms"] * 1e3)
        cum = ops.sgns_noise_table(walks, n)

        def fresh():
            return [ops.sgns_init(n, DIM, seed=0, device=dev)] + [torch.zeros(n, DIM, device=dev) for _ in range(3)]
        mine, theirs = fresh(), fresh()
        order = torch.empty(n_walks, dtype=torch.int32, device=dev)
        _lib.call("gae_sgns_walk_order", n_walks, 0, 0, _ptr(order), _stream())
        gen = torch.Generator(device=dev).manual_seed(0)
        epoch_no = [0]

        def epoch():
            ops.sgns_train(walks, cum, *mine, window=WINDOW, negatives=K, shared_negatives=M, epochs=1, batch_walks=BATCH, lr=LR,
                           eps=EPS, seed=0, first_epoch=epoch_no[0])
            epoch_no[0] += 1
        routes = {"epoch": epoch}
        if not a.no_torch:
            routes["epoch_torch"] = lambda: torch_epoch(walks, cum, *theirs, order, gen)
        row.update(timed(routes))
        if not a.no_torch:
            row["ratio_torch_over_epoch"] = row["epoch_torch"]["ms"] / row["epoch"]["ms"]

        # the two launches of one full batch, on the tables the epochs left
        AW, AC = (torch.zeros(n, DIM, dtype=torch.int64, device=dev) for _ in range(2))
        count = min(BATCH, n_walks)

        def accumulate():
            _lib.call("gae_sgns_accumulate", _ptr(walks), n_walks, L, _ptr(order), 0, count, _ptr(cum), n, DIM, WINDOW, K, M, 0, 99,
                      _ptr(mine[0]), _ptr(mine[1]), _ptr(AW), _ptr(AC), _ptr(status), _stream())

        def update():
            _lib.call("gae_sgns_update", _ptr(mine[0]), _ptr(mine[1]), _ptr(mine[2]), _ptr(mine[3]), _ptr(AW), _ptr(AC), n, DIM,
                      LR, EPS, _ptr(status), _stream())

        def before(route):                                                 # the sweep always meets one batch's accumulators
            if route == "update":
                AW.zero_(); AC.zero_()
                accumulate()
            else:
                AW.zero_(); AC.zero_()
        accumulate()
        touched = int((AW != 0).sum() + (AC != 0).sum())
        row.update(timed({"accumulate": accumulate, "update": update}, before))
        LP, dP = (L + 15) // 16 * 16, (DIM + 15) // 16 * 16
        flop = count * 2 * (LP * (LP + M) * dP + LP * (LP + M) * dP + (LP + M) * LP * dP)
        row["batch_matrix_flop"] = flop
        row["batch_matrix_us_at_peak"] = flop / FP32_MATRIX_FLOPS * 1e6
        row["accumulate_share_of_matrix_peak"] = row["batch_matrix_us_at_peak"] / (row["accumulate"]["ms"] * 1e3)
        sweep = 2 * n * DIM * 8 + touched * 16
        row["touched_elements"] = touched
        row["update_bytes_min"] = sweep
        row["update_gb_per_s"] = sweep / (row["update"]["ms"] * 1e-3) / 1e9
        row["update_share_of_copy_rate"] = sweep / HBM_COPY_BYTES_PER_S / (row["update"]["ms"] * 1e-3)
        row["epoch_update_bound_ms"] = row["n_batches"] * sweep / HBM_COPY_BYTES_PER_S * 1e3
        row["epoch_share_of_update_bound"] = row["epoch_update_bound_ms"] / row["epoch"]["ms"]
        row["epoch_matrix_ms_at_peak"] = n_walks / count * row["batch_matrix_us_at_peak"] * 1e-3
        row["status"] = int(status.cpu()[0])
        print(json.dumps(row), file=sys.stderr)
        rows.append(row)
        del g
        torch.cuda.empty_cache()
    result = {"what": "gae_random_walks on a preallocated table (walks_kernel) and ops.random_walks (walks_call); one epoch of "
                      "ops.sgns_train at ops.deepwalk's defaults (epoch) against the same schedule in torch (epoch_torch: gathers, "
                      "torch.bmm, index_add_, dense Adagrad); gae_sgns_accumulate and gae_sgns_update of one full batch alone; "
                      "device-event timings after warm-up, the series alternating call by call in one process; ms = median",
              "reps": a.reps, "warmup": a.warmup, "shapes": rows}
    text = json.dumps(result)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
