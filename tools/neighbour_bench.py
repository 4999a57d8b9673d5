#!/usr/bin/env python3
"""Neighbourhood link baselines (ops.neighbour_scores: gae_neighbour_pairs, K35; ops.neighbour_topk: gae_neighbour_topk, K36)
timed with device events after a warm-up on a Cora-sized and a Pubmed-sized graph with the planetoid degree profile (a few
hubs of 65 .. 171 neighbours) and on a random graph of 2 10^5 nodes with mean degree 10: 2 10^5 query pairs, the all-rows
top-10 for "aa" on the default route and with table_slots = 64 (every row with B_i > 32 on the window route).  Each is timed
twice: the entry point alone on preallocated outputs ("kernels"), and the whole wrapper call with its symmetry check,
allocations and status read ("call").
Beside each, alternating call by call, what a user would write today on the same device: ``torch.sparse.mm(A, A_weighted)``
with the weighted operand densified in column chunks so that every fp64 block stays under 1 GiB, then a gather of the query
pairs or a masked ``topk``.  The whole two-hop matrix passes through memory on that route, block by block.
Beside every kernel time stand the BYTES IT MUST WALK -- pairs: 4 (rowlen_i + rowlen_j) per pair plus 16 bytes of weights per
common neighbour; top-k: 4 B_i per row, B_i = sum of rowlen(w) over the neighbours w of i -- and the rate that makes.
The spread of every series is recorded: the machines are shared.  Prints one JSON object (and writes it with --out).
No time or ratio is a pass condition.

    python tools/neighbour_bench.py --out profiles/r26_neighbours.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GIB = 1 << 30
N_PAIRS = 200_000
K = 10


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


def planetoid_like(n, edges, hubs, seed):
    """undirected simple graph: `edges` random pairs plus hubs of the given degrees, both directions, no repeats"""
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n, edges), rng.integers(0, n, edges)
    for h, d in zip(rng.choice(n, len(hubs), replace=False), hubs):
        a = np.concatenate([a, np.full(d, h)])
        b = np.concatenate([b, rng.choice(n, d, replace=False)])
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    key = np.unique(lo[lo != hi] * n + hi[lo != hi])
    lo, hi = key // n, key % n
    return np.concatenate([lo, hi]), np.concatenate([hi, lo])


SHAPES = [("cora_like", 2708, 5000, (168, 99, 78, 74, 65)), ("pubmed_like", 19717, 43500, (171, 154, 129, 118, 103)),
          ("random_200k", 200_000, 1_000_000, ())]


def torch_two_hop(indptr, indices, w, n, visit):
    """the torch route: S[:, block] = A @ (diag(w) A[:, block]) by torch.sparse.mm on dense fp64 column blocks under
    1 GiB; visit(c0, c1, S_block) sees S[j, i - c0] for the query rows i of the block (A is symmetric)"""
    dev = indptr.device
    A = torch.sparse_csr_tensor(indptr.long(), indices.long(), torch.ones(indices.numel(), dtype=torch.float64, device=dev),
                                size=(n, n))
    chunk = max(1, min(n, GIB // (8 * n)))
    counts = (indptr[1:] - indptr[:-1]).long()
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        lo, hi = int(indptr[c0]), int(indptr[c1])
        cols = indices[lo:hi].long()
        rid = torch.repeat_interleave(torch.arange(c1 - c0, device=dev), counts[c0:c1])
        D = torch.zeros(n, c1 - c0, dtype=torch.float64, device=dev)
        D[cols, rid] = w[cols]
        visit(c0, c1, torch.sparse.mm(A, D))


def torch_pairs(indptr, indices, w, n, pi, pj):
    order = torch.argsort(pi)
    si, sj = pi[order], pj[order]
    out = torch.empty(pi.numel(), dtype=torch.float64, device=pi.device)

    def visit(c0, c1, S):
        lo, hi = int(torch.searchsorted(si, c0)), int(torch.searchsorted(si, c1))
        out[order[lo:hi]] = S[sj[lo:hi], si[lo:hi] - c0]
    torch_two_hop(indptr, indices, w, n, visit)
    return out


def torch_topk(indptr, indices, w, n, k):
    dev = indptr.device
    counts = (indptr[1:] - indptr[:-1]).long()
    idx = torch.empty(n, k, dtype=torch.int64, device=dev)
    val = torch.empty(n, k, dtype=torch.float64, device=dev)

    def visit(c0, c1, S):
        S = torch.where(S > 0, S, torch.full((), float("-inf"), dtype=torch.float64, device=dev))
        lo, hi = int(indptr[c0]), int(indptr[c1])
        rid = torch.repeat_interleave(torch.arange(c1 - c0, device=dev), counts[c0:c1])
        S[indices[lo:hi].long(), rid] = float("-inf")                      # known edges
        S[torch.arange(c0, c1, device=dev), torch.arange(c1 - c0, device=dev)] = float("-inf")
        v, i = torch.topk(S, k, dim=0)
        idx[c0:c1], val[c0:c1] = i.t(), v.t()
    torch_two_hop(indptr, indices, w, n, visit)
    return idx, val


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

    def timed(routes):
        times, out = {r: [] for r in routes}, {}
        for rep in range(a.warmup + a.reps):                               # alternating: every series sees the same neighbours
            for r, fn in routes.items():
                t = event_ms(lambda: out.__setitem__(r, fn()))
                if rep >= a.warmup:
                    times[r].append(t)
        return {r: series(times[r]) for r in routes}, out

    rows = []
    for name, n, edges, hubs in SHAPES:
        if name not in a.shapes:
            continue
        src, dst = planetoid_like(n, edges, hubs, seed=0)
        g = G.DGLGraph((src, dst), num_nodes=n).to(dev)
        indptr, indices = g.csr()
        nnz = indices.numel()
        deg, W = ops.neighbour_weights(g)
        rowlen = (indptr[1:] - indptr[:-1]).long()
        B = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(
            0, torch.repeat_interleave(torch.arange(n, device=dev), rowlen), rowlen[indices.long()])
        w_aa = torch.where(deg >= 2, 1.0 / torch.log(deg.double().clamp(min=2)), torch.zeros((), dtype=torch.float64, device=dev))
        gen = torch.Generator(device="cpu").manual_seed(1)
        pairs = torch.randint(0, n, (2, N_PAIRS), generator=gen).to(dev)
        pi, pj = pairs[0].to(torch.int32).contiguous(), pairs[1].to(torch.int32).contiguous()
        common = torch.empty(N_PAIRS, dtype=torch.int32, device=dev)
        wsum = torch.empty(N_PAIRS, 2, dtype=torch.int64, device=dev)
        status = torch.zeros(_lib.NEIGHBOUR_STATUS_WORDS, dtype=torch.int64, device=dev)
        index = torch.empty(n, K, dtype=torch.int32, device=dev)
        tcommon = torch.empty(n, K, dtype=torch.int32, device=dev)
        twsum = torch.empty(n, K, dtype=torch.int64, device=dev)
        ws = torch.empty(ops._ws_bytes("gae_neighbour_topk_workspace_bytes", n, n), dtype=torch.uint8, device=dev)

        def pairs_kernels():
            _lib.call("gae_neighbour_pairs", _ptr(indptr), _ptr(indices), n, nnz, _ptr(pi), _ptr(pj), N_PAIRS, _ptr(W), 2,
                      _ptr(common), _ptr(wsum), _ptr(status), _stream())

        def topk_kernels(slots):
            _lib.call("gae_neighbour_topk", _ptr(indptr), _ptr(indices), n, nnz, None, n, K, _lib.NEIGHBOUR_AA, W.data_ptr(), 2,
                      _ptr(deg), _lib.NEIGHBOUR_EXCLUDE_EDGES, slots, _ptr(index), _ptr(tcommon), _ptr(twsum), _ptr(status),
                      _ptr(ws), ws.numel(), _stream())

        row = {"case": name, "n": n, "nnz": nnz, "max_degree": int(deg.max()), "mean_degree": float(deg.double().mean()),
               "pairs": N_PAIRS, "k": K, "B_mean": float(B.double().mean()), "B_max": int(B.max()),
               "rows_long_default": int((2 * B > ops.NEIGHBOUR_TABLE_SLOTS).sum()), "rows_long_64": int((2 * B > 64).sum())}

        routes = {"pairs_kernels": pairs_kernels, "pairs_call": lambda: ops.neighbour_scores(g, pairs, weights=(deg, W))}
        if not a.no_torch:
            routes["pairs_torch_sparse_mm"] = lambda: torch_pairs(indptr, indices, w_aa, n, pairs[0], pairs[1])
        t, out = timed(routes)
        row.update(t)
        pair_bytes = int((4 * (rowlen[pairs[0]] + rowlen[pairs[1]])).sum()) + 16 * int(out["pairs_call"].common.sum())
        row["pairs_bytes"] = pair_bytes
        row["pairs_gb_per_s"] = pair_bytes / (row["pairs_kernels"]["ms"] * 1e-3) / 1e9
        if "pairs_torch_sparse_mm" in out:
            row["ratio_torch_over_pairs_call"] = row["pairs_torch_sparse_mm"]["ms"] / row["pairs_call"]["ms"]
            row["pairs_max_abs_diff_vs_torch"] = float((out["pairs_call"].aa - out["pairs_torch_sparse_mm"]).abs().max())

        routes = {"topk_kernels": lambda: topk_kernels(0), "topk_kernels_slots64": lambda: topk_kernels(64),
                  "topk_call": lambda: ops.neighbour_topk(g, K, "aa", weights=(deg, W)),
                  "topk_call_slots64": lambda: ops.neighbour_topk(g, K, "aa", weights=(deg, W), table_slots=64)}
        if not a.no_torch:
            routes["topk_torch_sparse_mm"] = lambda: torch_topk(indptr, indices, w_aa, n, K)
        t, out = timed(routes)
        row.update(t)
        row["topk_bytes"] = int(4 * B.sum())
        row["topk_gb_per_s"] = row["topk_bytes"] / (row["topk_kernels"]["ms"] * 1e-3) / 1e9
        row["topk_slots64_gb_per_s"] = row["topk_bytes"] / (row["topk_kernels_slots64"]["ms"] * 1e-3) / 1e9
        row["routes_equal"] = all(torch.equal(x, y) for x, y in zip(out["topk_call"], out["topk_call_slots64"]))
        if "topk_torch_sparse_mm" in out:
            row["ratio_torch_over_topk_call"] = row["topk_torch_sparse_mm"]["ms"] / row["topk_call"]["ms"]
            ti, tv = out["topk_torch_sparse_mm"]
            mine = out["topk_call"]
            both = (mine.index >= 0) & torch.isfinite(tv)
            row["topk_value_max_abs_diff_vs_torch"] = float((mine.value - tv)[both].abs().max())
            row["topk_index_equal_fraction_vs_torch"] = float((mine.index.long() == ti)[both].double().mean())   # ties differ
        print(json.dumps(row), file=sys.stderr)
        rows.append(row)
        del g
        torch.cuda.empty_cache()
    result = {"what": "gae_neighbour_pairs / gae_neighbour_topk (kind aa, k = 10, known edges excluded) on preallocated outputs "
                      "(*_kernels) and ops.neighbour_scores / ops.neighbour_topk as whole calls with weights= (*_call), against "
                      "torch.sparse.mm(A, diag(w) A) on dense fp64 column blocks under 1 GiB followed by a gather or a masked "
                      "topk; device-event timings after warm-up, the series alternating call by call in one process; ms = "
                      "median; *_gb_per_s = the bytes the kernel must walk over the kernels' time",
              "reps": a.reps, "warmup": a.warmup, "shapes": rows}
    text = json.dumps(result)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
