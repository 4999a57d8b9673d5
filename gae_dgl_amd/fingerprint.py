"""The ECFP rows of the reference's chemistry table from one command: circular fingerprints of a molecule set on the
device, their Tanimoto neighbours, and the table's heads on the folded counts.

  python -m gae_dgl_amd.fingerprint -d data/zinc.npz --out fp.npy
  python -m gae_dgl_amd.fingerprint --synthetic 20000 --out fp.npy --neighbours 10 --targets y.npy --ridge --forest

The fingerprint is ``ops.fingerprint_graphs`` (K33): a Morgan / Weisfeiler-Lehman hash over what the set stores, the
featuriser rows and the bonds.  The set holds no bond orders, so these are ECFP-LIKE descriptors, not RDKit's ECFP bits.
``--out`` receives int32 bit words [G, n_bits / 32] (``--counts``: int32 slot counts [G, n_bits]).
``--neighbours K`` runs the Tanimoto self-search on the bit words (``ops.tanimoto_knn``: the exact K most similar other
molecules of every molecule); ``--neighbours_out PATH`` writes 'index' int32 [G, K] and 'value' fp32 [G, K] as .npz; with
``--targets y.npy`` (one property per molecule) it prints the leave-one-out RMSE | MAE | R2 of the kNN regressor (uniform
weights), with ``--labels y.npy`` (integer classes, -1 = unlabelled) the leave-one-out accuracy.
``--ridge``, ``--forest [N_TREES]``, ``--mlp [H ...]`` fit the table's heads, each with its defaults, on the COUNT fingerprint
folded to min(n_bits, the head's width limit) columns (``ops.fingerprint_fold``; 128 for ridge and the MLP, 256 for the
forest) and print that head's line of ``gae_dgl_amd.embed`` behind the prefix ``ECFP-like (r = R, D counts)``; they need
``--targets`` ([G] or [G, t])."""
import argparse
import os
import time

import numpy as np
import torch

from gae_dgl_amd import ops
from gae_dgl_amd.embed import load_dataset


def build_parser():
    ap = argparse.ArgumentParser(description="Circular fingerprints of a molecule set, their Tanimoto neighbours and heads")
    ap.add_argument("--data_file", "-d", type=str, default=None, help="dataset (flat .npz of DeviceGraphDataset.save)")
    ap.add_argument("--synthetic", type=int, default=0, metavar="G",
                    help="generate G ZINC-shaped molecules instead of reading --data_file")
    ap.add_argument("--out", "-o", type=str, default=None, help="where the fingerprints go (.npy)")
    ap.add_argument("--n_bits", type=int, default=1024, metavar="N", help="slots: a power of two in 64..2048 (default 1024)")
    ap.add_argument("--radius", type=int, default=2, metavar="R", help="bonds around every atom, 0..8 (default 2)")
    ap.add_argument("--counts", action="store_true", help="write slot counts [G, N] instead of bit words [G, N / 32]")
    ap.add_argument("--neighbours", type=int, default=None, metavar="K",
                    help="also search the bit fingerprints against themselves: the K (1..64) most Tanimoto-similar other "
                         "molecules of every molecule, exact, on the device")
    ap.add_argument("--neighbours_out", type=str, default=None, metavar="PATH",
                    help="with --neighbours: write the lists (.npz: 'index' int32 [G, K], 'value' fp32 [G, K])")
    ap.add_argument("--targets", type=str, default=None, metavar="PATH",
                    help="a .npy of properties: with --neighbours one per molecule (the kNN regressor), with --ridge / "
                         "--forest / --mlp [G] or [G, t]")
    ap.add_argument("--labels", type=str, default=None, metavar="PATH",
                    help="with --neighbours: a .npy [G] of integer classes (-1 = unlabelled); prints the leave-one-out accuracy")
    ap.add_argument("--ridge", action="store_true", help="fit the ridge head (ops.ridge, its defaults) on the folded counts")
    ap.add_argument("--forest", type=int, nargs="?", const=100, default=None, metavar="N_TREES",
                    help="grow the random forest head (ops.forest, default 100 trees) on the folded counts")
    ap.add_argument("--mlp", type=int, nargs="*", default=None, metavar="H",
                    help="train the MLP head (ops.mlp, one or two hidden widths, default 100) on the folded counts")
    ap.add_argument("--seed", type=int, default=None, help="seed of --synthetic and of the heads")
    ap.add_argument("--gpu_id", type=int, default=0, help="which GPU")
    return ap


def parse_args(argv=None):
    """the arguments, checked: combinations that cannot work fail here, with a message, before any GPU is touched"""
    parser = build_parser()
    args = parser.parse_args(argv)
    if not args.out:
        parser.error("--out is required: the .npy file the fingerprints are written to")
    if bool(args.data_file) == bool(args.synthetic):
        parser.error("give exactly one of --data_file and --synthetic G")
    if args.synthetic < 0:
        parser.error("--synthetic takes a positive number")
    if args.n_bits not in ops.FINGERPRINT_N_BITS:
        parser.error(f"--n_bits {args.n_bits}: N must be one of {ops.FINGERPRINT_N_BITS}")
    if not 0 <= args.radius <= ops.FINGERPRINT_MAX_RADIUS:
        parser.error(f"--radius {args.radius}: R must lie in 0..{ops.FINGERPRINT_MAX_RADIUS}")
    heads = args.ridge or args.forest is not None or args.mlp is not None
    if args.neighbours is None:
        if args.neighbours_out or args.labels:
            parser.error("--neighbours_out / --labels need --neighbours K")
        if args.targets and not heads:
            parser.error("--targets needs --neighbours K or a head (--ridge / --forest / --mlp)")
    else:
        if not 1 <= args.neighbours <= ops.KNN_MAX_K:
            parser.error(f"--neighbours {args.neighbours}: K must lie in 1..{ops.KNN_MAX_K}")
    if heads and not args.targets:
        parser.error("--ridge / --forest / --mlp need --targets PATH: the property (or properties) to regress on")
    if args.forest is not None and not 1 <= args.forest <= ops.FOREST_MAX_TREES:
        parser.error(f"--forest {args.forest}: N_TREES must lie in 1..{ops.FOREST_MAX_TREES}")
    if args.mlp is not None:
        hidden = args.mlp or [100]
        if not 1 <= len(hidden) <= 2 or not all(1 <= h <= ops.MLP_MAX_WIDTH for h in hidden):
            parser.error(f"--mlp {' '.join(map(str, hidden))}: one or two hidden widths in 1..{ops.MLP_MAX_WIDTH}")
    for flag, path in (("--targets", args.targets), ("--labels", args.labels)):
        if path and not os.path.exists(path):
            parser.error(f"{flag} {path}: no such file")
    return args


def _head_targets(path, n, device):
    y = np.load(path)
    if y.ndim not in (1, 2) or y.shape[0] != n:
        raise ValueError(f"--targets of shape {y.shape} for {n} molecules: [G] or [G, t]")
    return torch.from_numpy(y.astype(np.float32)).to(device)


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("gae_dgl_amd runs on AMD GPUs only (no CPU fallback)")
    device = torch.device(f"cuda:{args.gpu_id}")
    torch.cuda.set_device(device)
    graphs = load_dataset(args, device)
    G, R, N = len(graphs), args.radius, args.n_bits
    print(f"Loaded {G} molecules")
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    fp = graphs.fingerprints(radius=R, n_bits=N, counts=args.counts)
    torch.cuda.synchronize(device)
    seconds = time.perf_counter() - t0
    out = fp.cpu().numpy()
    np.save(args.out, out)
    print(f"Fingerprinted {G} molecules -> {tuple(out.shape)} int32 {'counts' if args.counts else 'bit words'} "
          f"(ECFP-like, r = {R}, {N} bits; not RDKit's bits: the set stores no bond orders) | {seconds * 1e3:.3f} ms | "
          f"wrote {args.out}")
    main.fingerprints = fp
    main.neighbours = main.knn_scores = main.knn_accuracy = None
    if args.neighbours is not None:
        from gae_dgl_amd import metrics
        words = graphs.fingerprints(radius=R, n_bits=N) if args.counts else fp
        K = args.neighbours
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        nn = ops.tanimoto_knn(words, k=K)
        torch.cuda.synchronize(device)
        print(f"Searched {G} molecules for their {K} most similar (Tanimoto) | "
              f"{(time.perf_counter() - t0) * 1e3:.3f} ms (one call, set-up included)")
        main.neighbours = nn
        if args.neighbours_out:
            np.savez(args.neighbours_out, index=nn.index.cpu().numpy(), value=nn.value.cpu().numpy())
        head = f"ECFP-like (r = {R}, {N} bits) kNN ({K}, Tanimoto, leave-one-out)"
        if args.targets:
            y = np.load(args.targets)
            if y.shape[0] != G or (y.ndim > 1 and int(np.prod(y.shape[1:])) != 1):
                if not (args.ridge or args.forest is not None or args.mlp is not None):
                    raise ValueError(f"--targets of shape {y.shape} for the kNN regressor on {G} molecules: one property "
                                     f"per molecule")
                print(f"{head}: left out, --targets of shape {y.shape} holds more than one property per molecule")
            else:
                y = torch.from_numpy(y.reshape(-1).astype(np.float64)).to(device)
                rm = metrics.regression_metrics(metrics.knn_predict(nn.index, nn.value, y), y)
                print(f"{head} RMSE: {rm['rmse']:.6f} | MAE: {rm['mae']:.6f} | R2: {rm['r2']:.6f}")
                main.knn_scores = rm
        if args.labels:
            y = np.load(args.labels)
            if y.ndim != 1 or y.shape[0] != G or not np.issubdtype(y.dtype, np.integer):
                raise ValueError(f"--labels of shape {y.shape}, {y.dtype} for {G} molecules: integer classes [G]")
            y = torch.from_numpy(y.astype(np.int64)).to(device)
            pred = metrics.knn_predict(nn.index, nn.value, y, task="classification")
            scored = (y >= 0) & (pred >= 0)
            acc = float((pred[scored] == y[scored]).double().mean()) if bool(scored.any()) else float("nan")
            print(f"{head} accuracy: {acc:.4f} | molecules scored: {int(scored.sum())} of {G}")
            main.knn_accuracy = acc
    main.ridge = main.forest = main.mlp = None
    if args.ridge or args.forest is not None or args.mlp is not None:
        counts = fp if args.counts else graphs.fingerprints(radius=R, n_bits=N, counts=True)
        y = _head_targets(args.targets, G, device)
        seed = args.seed or 0

        def folded(limit):
            D = min(N, limit)
            return D, ops.fingerprint_fold(counts, D, counts=True).float()
    if args.ridge:
        D, X = folded(ops.RIDGE_MAX_D)
        res = ops.ridge(X, y, None, folds=5, seed=seed)
        chosen = res.lambdas.tolist().index(res.lam)
        pairs = " | ".join(f"RMSE: {r:.6f} | R2: {q:.6f}"
                           for r, q in zip(res.cv_rmse[chosen].tolist(), res.cv_r2[chosen].tolist()))
        print(f"ECFP-like (r = {R}, {D} counts) Ridge (5-fold CV, lambda = {res.lam:g}) {pairs}")
        main.ridge = res
    if args.forest is not None:
        D, X = folded(ops.FOREST_MAX_D)
        res = ops.forest(X, y, args.forest, seed=seed)
        pairs = " | ".join(f"RMSE: {r:.6f} | R2: {q:.6f}" for r, q in zip(res.oob_rmse.tolist(), res.oob_r2.tolist()))
        print(f"ECFP-like (r = {R}, {D} counts) Random Forest ({args.forest} trees, depth 12, out-of-bag) {pairs}")
        main.forest = res
    if args.mlp is not None:
        D, X = folded(ops.MLP_MAX_WIDTH)
        hidden = tuple(args.mlp or [100])
        res = ops.mlp(X, y, hidden, seed=seed)
        chosen = res.lrs.index(res.lr) * len(res.alphas) + res.alphas.index(res.alpha)
        pairs = " | ".join(f"RMSE: {r:.6f} | R2: {q:.6f}"
                           for r, q in zip(res.cv_rmse[chosen].tolist(), res.cv_r2[chosen].tolist()))
        print(f"ECFP-like (r = {R}, {D} counts) MLP ({' x '.join(map(str, hidden))}, 5-fold CV, lr = {res.lr:g}, "
              f"alpha = {res.alpha:g}) {pairs}")
        main.mlp = res
    return out


if __name__ == '__main__':
    main()
