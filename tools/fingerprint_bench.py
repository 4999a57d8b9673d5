#!/usr/bin/env python3
"""Circular fingerprints (ops.fingerprint_graphs: gae_fingerprint_graphs, K33) and the Tanimoto search over them
(ops.tanimoto_knn: gae_tanimoto_knn, K34) timed with device events after a warm-up on ``zinc_like`` sets of 1 128,
19 717 and 249 455 molecules: the fingerprint at radius 2 and 1024 bits, the self-search at k = 10 on each set, and
4 096 queries against the largest set at k = 64.  Beside the search, alternating call by call, the route a user would
otherwise write on the same device: unpack to fp16 0 / 1 columns, ``Q @ X.T`` over chunks of queries sized so that the
chunk x n matrix stays under 1 GiB, the quotient, ``topk``.
Beside every search time stands its ISSUE BOUND: an AND and an accumulating bit count per 32-bit word pair, 2 lane-ops,
so m n W 2 / (256 CUs x 4 SIMDs x 16 lanes x clock), and the fraction of it the kernel reaches.
The spread of every series is recorded: the machines are shared.  Prints one JSON object (and writes it with --out).
No time or ratio is a pass condition.

    python tools/fingerprint_bench.py --out profiles/r25_fingerprint.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETS = [1128, 19717, 249_455]
RADIUS, N_BITS = 2, 1024
LANES = 256 * 4 * 16              # CUs x SIMDs x lanes that issue per clock
GIB = 1 << 30


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def series(xs):
    xs = np.asarray(xs, dtype=np.float64)
    return {"ms": float(np.median(xs)), "ms_min": float(xs.min()), "ms_max": float(xs.max()), "reps": int(xs.size)}


def torch_tanimoto(Qw, Xw, k, same):
    """unpack -> fp16 product over query chunks under 1 GiB -> quotient -> topk"""
    from gae_dgl_amd import ops
    Xb = ops.fingerprint_unpack(Xw, torch.float16)
    Qb = Xb if same else ops.fingerprint_unpack(Qw, torch.float16)
    a, b = Qb.sum(1, dtype=torch.float32), Xb.sum(1, dtype=torch.float32)
    n = Xb.shape[0]
    chunk = max(1, GIB // (2 * n))
    idx, val = [], []
    for r0 in range(0, Qb.shape[0], chunk):
        c = (Qb[r0:r0 + chunk] @ Xb.t()).float()
        u = a[r0:r0 + chunk, None] + b[None, :] - c
        s = torch.where(u > 0, c / u, torch.zeros_like(c))
        if same:
            rows = torch.arange(s.shape[0], device=s.device)
            s[rows, rows + r0] = float("-inf")
        v, i = torch.topk(s, k, dim=1)
        idx.append(i); val.append(v)
    return torch.cat(idx), torch.cat(val)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sets", type=int, nargs="+", default=SETS)
    ap.add_argument("--no_torch", action="store_true", help="skip the torch route")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from gae_dgl_amd import ops
    from gae_dgl_amd.dataset import DeviceGraphDataset
    dev = torch.device("cuda:0")
    clock_hz = ops.device_info(0)["clock_khz"] * 1e3
    W = N_BITS // 32

    def search_row(name, Qw, Xw, k, same):
        m, n = Qw.shape[0], Xw.shape[0]
        routes = {"tanimoto_knn": lambda: ops.tanimoto_knn(Qw, None if same else Xw, k=k)}
        if not a.no_torch:
            routes["torch_unpack_matmul_topk"] = lambda: torch_tanimoto(Qw, Xw, k, same)
        times, out = {r: [] for r in routes}, {}
        for rep in range(a.warmup + a.reps):                           # alternating: every series sees the same neighbours
            for r, fn in routes.items():
                t = event_ms(lambda: out.__setitem__(r, fn()))
                if rep >= a.warmup:
                    times[r].append(t)
        row = {"case": name, "m": m, "n": n, "words": W, "k": k}
        for r in routes:
            row[r] = series(times[r])
        bound_ms = m * n * W * 2.0 / (LANES * clock_hz) * 1e3
        row["issue_bound_ms"] = bound_ms
        row["issue_bound_fraction"] = bound_ms / row["tanimoto_knn"]["ms"]
        if "torch_unpack_matmul_topk" in routes:
            row["ratio_torch_over_tanimoto_knn"] = row["torch_unpack_matmul_topk"]["ms"] / row["tanimoto_knn"]["ms"]
            ti, tv = out["torch_unpack_matmul_topk"]
            row["value_equal_fraction_vs_torch"] = float((out["tanimoto_knn"].value == tv).double().mean())
            row["index_equal_fraction_vs_torch"] = float((out["tanimoto_knn"].index.long() == ti).double().mean())
        print(json.dumps(row), file=sys.stderr)
        return row

    fingerprints, searches = [], []
    words = None
    for G in a.sets:
        data = DeviceGraphDataset.synthetic_zinc(G, seed=0, device=dev)
        hold = {}
        ts = [event_ms(lambda: hold.__setitem__("fp", data.fingerprints(radius=RADIUS, n_bits=N_BITS)))
              for _ in range(a.warmup + a.reps)][a.warmup:]
        words = hold["fp"]
        row = {"molecules": G, "atoms": data.n_nodes, "radius": RADIUS, "n_bits": N_BITS, **series(ts)}
        row["ns_per_atom"] = row["ms"] * 1e6 / max(data.n_nodes, 1)
        row["mean_bits_set"] = float(ops.fingerprint_unpack(words[:4096]).sum(1).mean())
        fingerprints.append(row)
        print(json.dumps(row), file=sys.stderr)
        del data
        searches.append(search_row(f"self_{G}", words, words, 10, True))
    if words is not None and words.shape[0] > 4096:
        g = torch.Generator(device="cpu").manual_seed(1)
        Q = words[torch.randperm(words.shape[0], generator=g)[:4096].to(dev)].contiguous()
        searches.append(search_row("queries_4096", Q, words, 64, False))
    result = {"what": "ops.fingerprint_graphs (the zeroing launch and one launch per radius; its allocations included) and "
                      "ops.tanimoto_knn (row bit counts, sweep, merge of the splits; its allocations included) on zinc_like "
                      "sets, against unpack -> fp16 Q @ X.T over query chunks under 1 GiB -> quotient -> topk in plain "
                      "torch; device-event timings of whole calls after warm-up, the series alternating call by call in "
                      "one process; ms = median; issue bound = m n W 2 lane-ops / (256 CUs x 4 SIMDs x 16 lanes x clock)",
              "clock_hz": clock_hz, "reps": a.reps, "warmup": a.warmup, "fingerprint": fingerprints, "search": searches}
    text = json.dumps(result)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
