#!/usr/bin/env python3
"""Exact t-SNE on the device (ops.tsne: gae_knn, gae_tsne_affinities, then gae_tsne_repulsion + gae_tsne_update per
iteration, K29) timed with device events after a warm-up on seeded data at Cora's size (n = 2 708, d = 16), Pubmed's
(n = 19 717, d = 16) and the molecule features of embed_graphs (n = 249 455, d = 48).  Reported per shape: microseconds
per iteration split over the launches (the repulsion sweep; reduce + update), the sweep against its VALU issue bound,
the affinity call, and the whole ops.tsne call (n_iter = 1000 / 250 / 20: the larger shapes run a REDUCED number of
iterations, the per-iteration time does not depend on it).  Beside them: the same schedule as plain torch on the device
(cdist-style row blocks under 1 GiB, index_add_ for the attraction), per iteration; and, where sklearn imports, its
TSNE(method="barnes_hut", n_jobs=16) on the host at the two smaller shapes -- a different, APPROXIMATE estimator (a
quad-tree at angle 0.5), timed for its own default schedule at n = 2 708 and for 250 iterations at n = 19 717.  The
spread of every series is recorded: the machines are shared.  Prints one JSON object (and writes it with --out).  No
time or ratio is a pass condition.

    python tools/tsne_bench.py --out profiles/r19_tsne.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = [("cora_z", 2708, 16, 1000), ("pubmed_z", 19717, 16, 250), ("zinc_features", 249_455, 48, 20)]
PERPLEXITY = 20.0
# the compiled inner loops of tsne_repulsion_kernel<R> (hipcc -S, the loop without the j = i predicate): VALU issue
# slots of 4 cycles per pair -- R = 4: 88 plain (v_pk_* count once) + 16 v_rcp_f32 at 2 slots for 16 pairs = 7.5
SLOTS_PER_PAIR = 7.5
LANES_PER_CLOCK = 256 * 4 * 16         # CUs x SIMDs x lanes a 4-cycle slot covers per cycle
CLOCK = 2.4e9


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def series(xs, scale=1.0, unit="ms"):
    xs = np.asarray(xs, dtype=np.float64) * scale
    return {unit: float(np.median(xs)), unit + "_min": float(xs.min()), unit + "_max": float(xs.max()), "reps": int(xs.size)}


def make(n, d, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    centres = torch.randn(7, d, generator=g) * 2.0
    return centres[torch.arange(n) % 7] + torch.randn(n, d, generator=g)


def torch_iteration(Y, rows, cols, vals, vel, gains, alpha, mu, eta, block):
    """one iteration of the same schedule in plain torch: row blocks of the n x n terms, nothing kept"""
    n = Y.shape[0]
    rep = torch.empty_like(Y)
    Z = torch.zeros((), device=Y.device)
    for r0 in range(0, n, block):
        r1 = min(r0 + block, n)
        dx = Y[r0:r1, 0:1] - Y[:, 0].unsqueeze(0)
        dy = Y[r0:r1, 1:2] - Y[:, 1].unsqueeze(0)
        q = 1.0 / (1.0 + dx * dx + dy * dy)
        q[torch.arange(r1 - r0, device=Y.device), torch.arange(r0, r1, device=Y.device)] = 0.0
        Z = Z + q.sum()
        q = q * q
        rep[r0:r1, 0] = (q * dx).sum(1)
        rep[r0:r1, 1] = (q * dy).sum(1)
    diff = Y[rows] - Y[cols]
    w = vals / (1.0 + (diff * diff).sum(1))
    attr = torch.zeros_like(Y).index_add_(0, rows, w.unsqueeze(1) * diff)
    g = 4.0 * (alpha * attr - rep / Z)
    gains = torch.where(torch.sign(g) != torch.sign(vel), gains + 0.2, gains * 0.8).clamp_min(0.01)
    vel = mu * vel - eta * gains * g
    return Y + vel, vel, gains


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--case", choices=[c[0] for c in CASES], default=None, help="one shape only")
    ap.add_argument("--no_torch", action="store_true", help="skip the torch route")
    ap.add_argument("--no_sklearn", action="store_true", help="skip sklearn's Barnes-Hut t-SNE on the host")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from gae_dgl_amd import ops
    dev = torch.device("cuda:0")
    result = {"device": ops.device_info(0)["name"], "perplexity": PERPLEXITY, "slots_per_pair": SLOTS_PER_PAIR, "cases": {}}
    for name, n, d, n_iter in CASES:
        if args.case and name != args.case:
            continue
        X = make(n, d, 1).to(dev)
        row = {"n": n, "d": d, "n_iter": n_iter, "chunk": ops.tsne_chunk(n)}
        nb = ops.knn(X, k=60)
        p, _ = ops.tsne_affinities(nb.index, nb.value, PERPLEXITY)
        indptr, indices, values = ops.tsne_symmetrise(nb.index, p)
        row["nnz"] = int(values.numel())
        reps = range(args.warmup + args.reps)
        row["knn"] = series([event_ms(lambda: ops.knn(X, k=60)) for _ in reps][args.warmup:])
        row["affinities"] = series([event_ms(lambda: ops.tsne_affinities(nb.index, nb.value, PERPLEXITY)) for _ in reps][args.warmup:])
        row["symmetrise"] = series([event_ms(lambda: ops.tsne_symmetrise(nb.index, p)) for _ in reps][args.warmup:])
        # the launches of an iteration, on a state part way into a run (the start has every q = 1)
        st = ops.TSNEState(ops.tsne_init(n, 0, dev), indptr, indices, values)
        eta = max(n / 48.0, 50.0)
        for _ in range(10):
            st.step(12.0, 0.5, eta)
        inner = 20 if n < 100_000 else 5
        row["repulsion"] = series([event_ms(lambda: [st.repulsion(gated=False) for _ in range(inner)]) for _ in reps][args.warmup:],
                                  1e3 / inner, "us")
        row["reduce_update"] = series([event_ms(lambda: [st.update(12.0, 0.5, eta) for _ in range(inner)]) for _ in reps][args.warmup:],
                                      1e3 / inner, "us")
        row["iteration"] = series([event_ms(lambda: [st.step(12.0, 0.5, eta) for _ in range(inner)]) for _ in reps][args.warmup:],
                                  1e3 / inner, "us")
        bound_us = SLOTS_PER_PAIR * float(n) * n / (LANES_PER_CLOCK * CLOCK) * 1e6
        row["repulsion_bound_us"] = bound_us
        row["repulsion_fraction_of_bound"] = bound_us / row["repulsion"]["us"]
        del st
        walls = []
        for _ in reps:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = ops.tsne(X, perplexity=PERPLEXITY, n_iter=n_iter, neighbours=None)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        row["tsne_call"] = series(walls[args.warmup:])
        row["kl_divergence"] = res.kl_divergence
        if not args.no_torch:
            rows = torch.repeat_interleave(torch.arange(n, device=dev), (indptr[1:] - indptr[:-1]).long())
            cols = indices.long()
            block = max(1, min(n, (1 << 30) // (32 * n)))                  # ~8 fp32 temporaries of block x n under 1 GiB
            Y = ops.tsne_init(n, 0, dev)
            state = [Y, torch.zeros_like(Y), torch.ones_like(Y)]

            def one():
                state[0], state[1], state[2] = torch_iteration(state[0], rows, cols, values, state[1], state[2], 12.0, 0.5, eta, block)
            row["torch_iteration"] = series([event_ms(one) for _ in reps][args.warmup:], 1e3, "us")
            row["torch_block_rows"] = block
            row["torch_over_ours"] = row["torch_iteration"]["us"] / row["iteration"]["us"]
        if not args.no_sklearn and n < 100_000:
            try:
                from sklearn.manifold import TSNE
            except ImportError:
                TSNE = None
            if TSNE is not None:
                kw = {} if n < 10_000 else {"max_iter": 250}
                t0 = time.perf_counter()
                est = TSNE(method="barnes_hut", n_jobs=16, perplexity=PERPLEXITY, init="random", random_state=0, **kw)
                est.fit(X.cpu().numpy())
                row["sklearn_barnes_hut"] = {"s": time.perf_counter() - t0, "n_iter": int(est.n_iter_), "kl": float(est.kl_divergence_),
                                             "note": "host, approximate (angle 0.5), its own schedule"}
        result["cases"][name] = row
        print(name, json.dumps(row), flush=True)
    text = json.dumps(result)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
