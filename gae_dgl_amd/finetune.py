"""Fine-tune a pre-trained encoder on a molecular property through the molecule feature of the reference's chemistry
table (README.md:54: mean | sum | max of the hidden vectors; the "GAE + MLP" row of its ESOL table, with the encoder no
longer frozen):

  python -m gae_dgl_amd.finetune --checkpoint result/ep09.pkl --hidden_dims 32 16 -d data/graphs.npz --targets y.npy \
      --head mlp --epochs 20 -b 4096 --lr 1e-3 --out result/finetuned

The checkpoint is the state dict ``train_inductive`` (and the reference's Trainer.save) writes; ``--targets`` a .npy with
one number per molecule of the dataset.  A torch head (``linear``: Linear(3 d, 1); ``mlp``: Linear(3 d, 64), ReLU,
Linear(64, 1)) sits on the 3 d-wide feature; head and encoder are trained with MSE and Adam through
``GAE.embed_graphs(grad=True)`` on ``subset()`` views of the resident set: forward and backward of the encoder are one
fused launch each (K19 / K21) wherever both kernels take the molecules, the chunked differentiable route elsewhere.
``--freeze_encoder`` trains the head alone (the reference's frozen-feature setting).  Prints the train loss per epoch;
writes ``encoder.pkl`` (the reference's state-dict keys, loadable by train_inductive / embed) and ``head.pkl`` to
``--out``.  ``--head_init model.npz`` (with ``--head mlp``) starts the head from the model ``embed --mlp_out`` saved (``ops.mlp``
trained it on the frozen features; its scaling is folded into the first and last layer) instead of a random
Linear(3 d, 64), ReLU, Linear(64, 1).  Plain host code: the head's GEMMs are torch's."""
import argparse
import os

import numpy as np
import torch
import torch.nn as nn

from gae_dgl_amd.dataset import DeviceGraphDataset
from gae_dgl_amd.gae import GAE


def build_parser():
    ap = argparse.ArgumentParser(description="Fine-tune a pre-trained GAE encoder on a molecular property")
    ap.add_argument("--checkpoint", "-c", type=str, default=None, help="state dict written by train_inductive (ep{NN}.pkl)")
    ap.add_argument("--hidden_dims", type=int, nargs="+", metavar="N", help="encoder widths, e.g. 32 16")
    ap.add_argument("--in_dim", "-i", type=int, default=39, help="atom feature width")
    ap.add_argument("--data_file", "-d", type=str, default=None, help="dataset (flat .npz of DeviceGraphDataset.save)")
    ap.add_argument("--synthetic", type=int, default=0, metavar="G",
                    help="generate G ZINC-shaped molecules instead of reading --data_file")
    ap.add_argument("--targets", "-t", type=str, default=None, help=".npy with one target per molecule")
    ap.add_argument("--head", choices=["linear", "mlp"], default="linear")
    ap.add_argument("--head_init", type=str, default=None, metavar="PATH",
                    help="with --head mlp: start the head from the .npz that `embed --mlp_out` wrote")
    ap.add_argument("--freeze_encoder", action="store_true", help="train the head alone on frozen features")
    ap.add_argument("--epochs", "-e", type=int, default=10)
    ap.add_argument("--batch_size", "-b", type=int, default=4096, help="molecules per step")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--norm", choices=["none", "both"], default="none")
    ap.add_argument("--fused", choices=["auto", "on", "off"], default="auto",
                    help="on = the kernel pair or an error; off = the chunked differentiable route; auto = the kernels "
                         "for every molecule both take")
    ap.add_argument("--out", "-o", type=str, default=None, help="directory for encoder.pkl and head.pkl")
    ap.add_argument("--seed", type=int, default=None, help="seed of the head's init, the shuffling and --synthetic")
    ap.add_argument("--gpu_id", type=int, default=0, help="which GPU")
    return ap


def parse_args(argv=None):
    """the arguments, checked: combinations that cannot work fail here, with a message, before any GPU is touched"""
    parser = build_parser()
    args = parser.parse_args(argv)
    if not args.checkpoint:
        parser.error("--checkpoint is required: the state dict train_inductive saved (ep{NN}.pkl)")
    if not args.hidden_dims:
        parser.error("--hidden_dims is required: the encoder widths the checkpoint was trained with, e.g. 32 16")
    if not args.targets:
        parser.error("--targets is required: a .npy with one number per molecule")
    if not args.out:
        parser.error("--out is required: the directory encoder.pkl and head.pkl are written to")
    if bool(args.data_file) == bool(args.synthetic):
        parser.error("give exactly one of --data_file and --synthetic G")
    if args.synthetic < 0 or args.batch_size < 1 or args.in_dim < 1 or min(args.hidden_dims) < 1 or args.epochs < 1:
        parser.error("--synthetic, --batch_size, --in_dim, --epochs and --hidden_dims take positive numbers")
    if not args.lr > 0:
        parser.error("--lr takes a positive number")
    if args.head_init:
        if args.head != "mlp":
            parser.error("--head_init needs --head mlp: it holds an MLP head")
        if not os.path.exists(args.head_init):
            parser.error(f"--head_init {args.head_init}: no such file")
    if args.fused == "on" and not args.freeze_encoder:
        from gae_dgl_amd import ops
        if not ops.embed_graphs_bwd_usable(args.in_dim, args.hidden_dims, 0):
            parser.error(f"--fused on: the backward kernel does not take {args.in_dim} -> {args.hidden_dims}; use "
                         f"--fused auto or off, or --freeze_encoder")
    return args


def make_head(kind, width):
    if kind == "linear":
        return nn.Linear(width, 1)
    return nn.Sequential(nn.Linear(width, 64), nn.ReLU(), nn.Linear(64, 1))


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("gae_dgl_amd runs on AMD GPUs only (no CPU fallback)")
    device = torch.device(f"cuda:{args.gpu_id}")
    torch.cuda.set_device(device)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    model = GAE(args.in_dim, args.hidden_dims, norm=None if args.norm == "none" else args.norm)
    model.load_state_dict(torch.load(args.checkpoint, map_location="cpu"))
    model = model.to(device)
    if args.synthetic:
        graphs = DeviceGraphDataset.synthetic_zinc(args.synthetic, seed=args.seed or 0, device=device)
    else:
        if not os.path.exists(args.data_file):
            raise FileNotFoundError(f"{args.data_file} not found (use --synthetic G for ZINC-shaped synthetic data)")
        graphs = DeviceGraphDataset.load(args.data_file, device=device)
    y = np.asarray(np.load(args.targets), dtype=np.float32).reshape(-1)
    if len(y) != len(graphs):
        raise ValueError(f"{args.targets} holds {len(y)} targets, the dataset {len(graphs)} molecules")
    y = torch.from_numpy(y).to(device)
    print(f"Loaded {len(graphs)} molecules")
    if args.head_init:
        from gae_dgl_amd import ops
        head = ops.mlp_load_head(args.head_init)
        if head[0].in_features != 3 * args.hidden_dims[-1] or head[-1].out_features != 1:
            raise ValueError(f"{args.head_init} holds a head {head[0].in_features} -> ... -> {head[-1].out_features}, the "
                             f"feature is {3 * args.hidden_dims[-1]} wide and there is one target")
        head = head.to(device)
    else:
        head = make_head(args.head, 3 * args.hidden_dims[-1]).to(device)
    for p in model.parameters():
        p.requires_grad_(not args.freeze_encoder)
    params = list(head.parameters()) + ([] if args.freeze_encoder else list(model.parameters()))
    opt = torch.optim.Adam(params, lr=args.lr)
    fused = {"auto": "auto", "on": True, "off": False}[args.fused]
    rng = np.random.default_rng(args.seed)
    G = len(graphs)
    losses = []
    for epoch in range(args.epochs):
        order = rng.permutation(G)
        total = torch.zeros((), dtype=torch.float64, device=device)
        for lo in range(0, G, args.batch_size):
            ids = np.sort(order[lo:lo + args.batch_size])
            feats = model.embed_graphs(graphs.subset(ids), fused=fused, batch_size=args.batch_size,
                                       grad=not args.freeze_encoder)
            pred = head(feats).squeeze(1)
            loss = torch.nn.functional.mse_loss(pred, y[torch.from_numpy(ids).to(device)])
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            total += loss.detach().double() * len(ids)
        losses.append(float(total) / G)
        print(f"Epoch: {epoch:02d} | train MSE {losses[-1]:.6f}")
    os.makedirs(args.out, exist_ok=True)
    torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, os.path.join(args.out, "encoder.pkl"))
    torch.save({k: v.detach().cpu() for k, v in head.state_dict().items()}, os.path.join(args.out, "head.pkl"))
    print(f"Wrote {os.path.join(args.out, 'encoder.pkl')} and head.pkl")
    main.losses, main.model, main.head = losses, model, head
    return losses


if __name__ == '__main__':
    main()
