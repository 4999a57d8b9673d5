"""Turn a pre-trained checkpoint into the molecule features of the reference's chemistry table (README.md:54: "GAE
feature is a concatenation of mean, sum, and max aggregation of the hidden vector", 48 numbers per molecule for
``--hidden_dims 32 16``):

  python -m gae_dgl_amd.embed --checkpoint result/ep09.pkl --hidden_dims 32 16 -d data/zinc.npz --out features.npy
  python -m gae_dgl_amd.embed --checkpoint result/ep09.pkl --hidden_dims 32 16 --synthetic 20000 --out features.npy

The checkpoint is the state dict ``train_inductive`` (and the reference's Trainer.save, train_inductive.py:56-57)
writes.  The whole set is embedded by ``GAE.embed_graphs``: one fused launch where the kernel takes the shapes
(``--fused auto|on``), the chunked batch -> encode -> readout route otherwise (``--fused off``).  Writes fp32
[G, 3 d] as .npy and prints the graph count, the route taken and the time of the embedding call.
``--scores PATH`` also writes how well each molecule is reconstructed (``GAE.score_graphs``): fp64 [G, 5] .npy with the
columns loss, auc, ap, n_pos, n_neg; the feature output is the same with and without it.
``--clusters K`` clusters the molecule features just computed with k-means on the device (``ops.kmeans``): chemical-space
clusters of the resident set; ``--clusters_out PATH`` writes 'labels' int32 [G] and 'centers' fp32 [K, 3 d] as .npz.
``--neighbours K`` searches the features just computed against themselves (``ops.knn``: the exact K nearest other
molecules of every molecule, ``--metric l2|dot|cosine``) and prints the time of that one call, first-use set-up included; ``--neighbours_out PATH``
writes 'index' int32 [G, K] and 'value' fp32 [G, K] as .npz; ``--targets y.npy`` (one property per molecule) prints the
leave-one-out RMSE | MAE | R2 of the kNN regressor on the frozen features.
``--ridge [LAMBDA ...]`` fits the reference table's "GAE + Ridge" head on the features just computed (``ops.ridge``: per-fold
fp64 moments in one pass over the features, lambda chosen by ``--ridge_folds F``-fold CV on the device; no values = the
default grid 10^-3 .. 10^3); needs ``--targets`` ([G] or [G, t]); prints the time of the call and the cross-validated
RMSE | R2 at the chosen lambda, one pair per target; ``--ridge_out PATH`` writes 'coef', 'intercept', 'lam', 'lambdas',
'cv_rmse' and 'cv_r2' as .npz.
``--forest [N_TREES]`` grows the table's "GAE + Random Forest" head on the features just computed (``ops.forest``: histogram
trees on the device, default 100 trees; ``--forest_depth D`` (default 12), ``--forest_features M`` features per split
(default all)); needs ``--targets`` ([G] or [G, t]); prints the time of the call and the out-of-bag RMSE | R2, one pair
per target; ``--forest_out PATH`` writes the node tables, 'edges', 'n_edges', 'oob_prediction', 'oob_rmse', 'oob_r2' and
'importances' as .npz.  Combines with ``--ridge`` and ``--neighbours``.
``--mlp [H ...]`` trains the table's "GAE + MLP" head on the features just computed (``ops.mlp``: one block per model, every
fold model of every (lr, alpha) pair side by side; hidden widths ``H`` (one or two, default 100); ``--mlp_epochs E`` (200),
``--mlp_batch B`` (200), ``--mlp_lr LR ...`` (1e-3), ``--mlp_alpha A ...`` (1e-4), ``--mlp_folds F`` (5), ``--mlp_ensemble S``
(1)); needs ``--targets`` ([G] or [G, t]); prints the time of the call and the cross-validated RMSE | R2 at the chosen
pair, one pair per target; ``--mlp_out PATH`` writes 'hidden', 'lr', 'alpha', 'shift', 'scale', 'cv_rmse', 'cv_r2' and per
layer 'weight{l}' [S, out, in], 'bias{l}' [S, out] as .npz (``finetune --head_init`` reads it).  Combines with ``--ridge``,
``--forest`` and ``--neighbours``.
``--labels y.npy --logreg [LAMBDA ...]`` fits the head of a classification property on the features just computed
(``ops.logreg``: multinomial logistic regression, every fold x lambda model in the same launches, lambda chosen by
``--logreg_folds F``-fold CV on the device; classes are integers, -1 = unlabelled) and prints accuracy | macro-F1 | log-loss
of the pooled held-out predictions at the chosen lambda; ``--logreg_out PATH`` writes 'coef', 'intercept', 'pivot', 'lam',
'lambdas', 'cv_logloss' and 'cv_accuracy' as .npz.  Combines with ``--ridge``, ``--forest``, ``--mlp`` and ``--neighbours``.
``--map_out map.npz`` maps the features just computed into the plane (``ops.tsne``: exact t-SNE on the device,
``--map_perplexity P`` (20), ``--map_iters T`` (1000), ``--map_seed S`` (0)), prints the KL divergence and the 10-NN
preservation of the map and writes 'embedding' [G, 2], 'labels' (those of ``--labels``, else -1), 'kl_divergence' and
'kl_curve'.  ``--map_init pca`` starts the map from the first two principal scores (sklearn's rule) instead of the Philox
draw.  Combines with every flag above.
``--pca K`` takes the K leading principal components of the features just computed (``ops.pca``: exact-order fp64 moments
in one pass, an fp64 Jacobi eigensolver in one block, the same bits run to run; ``--pca_whiten`` scales every score to unit
variance), prints the explained variance and, with ``--pca_out pca.npz``, writes 'components' [K, 3 d], 'mean', 'explained_variance',
'explained_variance_ratio' and 'scores' [G, K].  Combines with every flag above."""
import argparse
import os
import time

import numpy as np
import torch

from gae_dgl_amd import _lib, ops
from gae_dgl_amd.dataset import DeviceGraphDataset
from gae_dgl_amd.gae import GAE


def build_parser():
    ap = argparse.ArgumentParser(description="Embed a molecule set with a pre-trained GAE")
    ap.add_argument("--checkpoint", "-c", type=str, default=None, help="state dict written by train_inductive (ep{NN}.pkl)")
    ap.add_argument("--hidden_dims", type=int, nargs="+", metavar="N", help="encoder widths, e.g. 32 16")
    ap.add_argument("--in_dim", "-i", type=int, default=39, help="atom feature width")
    ap.add_argument("--data_file", "-d", type=str, default=None, help="dataset (flat .npz of DeviceGraphDataset.save)")
    ap.add_argument("--synthetic", type=int, default=0, metavar="G",
                    help="generate G ZINC-shaped molecules instead of reading --data_file")
    ap.add_argument("--out", "-o", type=str, default=None, help="where the [G, 3 d] fp32 features go (.npy)")
    ap.add_argument("--scores", type=str, default=None, metavar="PATH",
                    help="also write the per-molecule reconstruction scores (.npy, [G, 5] fp64: loss, auc, ap, n_pos, "
                         "n_neg)")
    ap.add_argument("--clusters", type=int, default=None, metavar="K",
                    help="also cluster the features with k-means (K in 1..256, on the device; 3 d <= 64) and print the "
                         "inertia, the iterations and the cluster sizes")
    ap.add_argument("--clusters_out", type=str, default=None, metavar="PATH",
                    help="with --clusters: write the labels and centres (.npz: 'labels' int32 [G], 'centers' fp32 [K, 3 d])")
    ap.add_argument("--neighbours", type=int, default=None, metavar="K",
                    help="also search the features against themselves: the K (1..64) nearest other molecules of every "
                         "molecule, exact, on the device (3 d <= 256); prints the time of the one call made (its "
                         "first-use set-up included: tools/knn_bench.py times warm calls)")
    ap.add_argument("--metric", choices=["l2", "dot", "cosine"], default=None,
                    help="with --neighbours: squared Euclidean distance (default), inner product or cosine similarity")
    ap.add_argument("--neighbours_out", type=str, default=None, metavar="PATH",
                    help="with --neighbours: write the lists (.npz: 'index' int32 [G, K], 'value' fp32 [G, K])")
    ap.add_argument("--targets", type=str, default=None, metavar="PATH",
                    help="with --neighbours: a .npy of one property per molecule; prints the leave-one-out RMSE | MAE | "
                         "R2 of the kNN regressor (mean of the K neighbours' targets).  With --ridge: [G] or [G, t], the "
                         "targets of the ridge head")
    ap.add_argument("--ridge", type=float, nargs="*", default=None, metavar="LAMBDA",
                    help="also fit a ridge regression head on the features (needs --targets; 3 d <= 128): the penalty "
                         "is chosen among the given values (none given: 10^-3 .. 10^3, 13 values) by k-fold CV on the "
                         "device; prints the cross-validated RMSE | R2")
    ap.add_argument("--ridge_folds", type=int, default=None, metavar="F", help="with --ridge: CV folds, 2..32 (default 5)")
    ap.add_argument("--ridge_out", type=str, default=None, metavar="PATH",
                    help="with --ridge: write the model (.npz: 'coef' [t, 3 d], 'intercept' [t], 'lam', 'lambdas', "
                         "'cv_rmse' [L, t], 'cv_r2' [L, t])")
    ap.add_argument("--forest", type=int, nargs="?", const=100, default=None, metavar="N_TREES",
                    help="also grow a random forest regression head on the features (needs --targets; 3 d <= 256): "
                         "N_TREES histogram trees (default 100) on the device; prints the out-of-bag RMSE | R2")
    ap.add_argument("--forest_depth", type=int, default=None, metavar="D", help="with --forest: depth limit, 1..16 (default 12)")
    ap.add_argument("--forest_features", type=int, default=None, metavar="M",
                    help="with --forest: features looked at per split, 1..3 d (default all)")
    ap.add_argument("--forest_out", type=str, default=None, metavar="PATH",
                    help="with --forest: write the model (.npz: the node tables 'feature', 'threshold_bin', 'threshold', "
                         "'left', 'count', 'value', 'gain', 'n_nodes', and 'edges', 'n_edges', 'oob_prediction', "
                         "'oob_rmse', 'oob_r2', 'importances')")
    ap.add_argument("--mlp", type=int, nargs="*", default=None, metavar="H",
                    help="also train an MLP regression head on the features (needs --targets; 3 d <= 128): one or two "
                         "hidden widths in 1..128 (none given: 100); the (lr, alpha) pair is chosen by k-fold CV on the "
                         "device; prints the cross-validated RMSE | R2")
    ap.add_argument("--mlp_epochs", type=int, default=None, metavar="E", help="with --mlp: epochs (default 200)")
    ap.add_argument("--mlp_batch", type=int, default=None, metavar="B", help="with --mlp: mini-batch size (default 200)")
    ap.add_argument("--mlp_lr", type=float, nargs="+", default=None, metavar="LR", help="with --mlp: learning rates (default 1e-3)")
    ap.add_argument("--mlp_alpha", type=float, nargs="+", default=None, metavar="A", help="with --mlp: L2 penalties (default 1e-4)")
    ap.add_argument("--mlp_folds", type=int, default=None, metavar="F", help="with --mlp: CV folds, 2..32 (default 5)")
    ap.add_argument("--mlp_ensemble", type=int, default=None, metavar="S", help="with --mlp: members per model (default 1)")
    ap.add_argument("--mlp_out", type=str, default=None, metavar="PATH",
                    help="with --mlp: write the chosen model (.npz: 'hidden', 'lr', 'alpha', 'shift', 'scale', 'cv_rmse', "
                         "'cv_r2', 'weight{l}', 'bias{l}')")
    ap.add_argument("--labels", type=str, default=None, metavar="PATH",
                    help="with --logreg: .npy file [G] of integer classes in the order of --out (-1 = unlabelled)")
    ap.add_argument("--logreg", type=float, nargs="*", default=None, metavar="LAMBDA",
                    help="also fit a multinomial logistic regression head on the features (needs --labels; 3 d <= 128, at "
                         "most 32 classes): the penalty is chosen by k-fold CV among the LAMBDAs (default 10^-3 .. 10^3, "
                         "13 values), all on the device; prints accuracy | macro-F1 | log-loss of the held-out predictions")
    ap.add_argument("--logreg_folds", type=int, default=None, metavar="F", help="with --logreg: CV folds, 2..32 (default 5)")
    ap.add_argument("--logreg_out", type=str, default=None, metavar="PATH",
                    help="with --logreg: write the model (.npz: 'coef' [c, 3 d], 'intercept' [c], 'pivot', 'lam', 'lambdas', "
                         "'cv_logloss', 'cv_accuracy')")
    ap.add_argument("--boost", type=int, nargs="?", const=100, default=None, metavar="N_ROUNDS",
                    help="also fit gradient-boosted histogram trees on the features (3 d <= 256), N_ROUNDS rounds at most "
                         "(default 100), on the device: with --targets PATH ([G], one property) the squared objective, "
                         "prints the RMSE | R2 of the held-out predictions; with --labels PATH (classes 0 / 1, -1 = "
                         "unlabelled) the logistic objective, prints accuracy | ROC-AUC | log-loss; the learning rate, "
                         "lambda and the number of rounds are chosen by k-fold CV")
    ap.add_argument("--boost_depth", type=int, default=None, metavar="D", help="with --boost: depth limit, 1..8 (default 4)")
    ap.add_argument("--boost_lr", type=float, nargs="+", default=None, metavar="LR",
                    help="with --boost: learning rates in (0, 1] (default 0.1)")
    ap.add_argument("--boost_lambda", type=float, nargs="+", default=None, metavar="L",
                    help="with --boost: L2 penalties of the leaf weights (default 1)")
    ap.add_argument("--boost_folds", type=int, default=None, metavar="F", help="with --boost: CV folds, 2..32 (default 5)")
    ap.add_argument("--boost_out", type=str, default=None, metavar="PATH",
                    help="with --boost: write the model (.npz: the node tables 'feature', 'threshold_bin', 'threshold', "
                         "'left', 'count', 'value', 'gain', 'n_nodes', and 'edges', 'n_edges', 'base_score', 'lr', 'lam', "
                         "'best_round', 'cv_curve', 'importances'; with both --targets and --labels the logistic model)")
    ap.add_argument("--map_out", type=str, default=None, metavar="PATH",
                    help="the 2-D map of the features by exact t-SNE on the device (ops.tsne) and its 10-NN preservation; "
                         "writes PATH (.npz: 'embedding' fp32 [G, 2], 'labels' int64 [G] (--labels, else -1), "
                         "'kl_divergence', 'kl_curve')")
    ap.add_argument("--map_perplexity", type=float, default=None, metavar="P",
                    help="with --map_out: the perplexity, at least 1 and below min(G - 1, 64) (default 20)")
    ap.add_argument("--map_iters", type=int, default=None, metavar="T", help="with --map_out: iterations (default 1000)")
    ap.add_argument("--map_seed", type=int, default=None, metavar="S", help="with --map_out: the seed of the start (default 0)")
    ap.add_argument("--map_init", choices=["random", "pca"], default=None,
                    help="with --map_out: the start of the map, the library's Philox draw (default) or the first two principal "
                         "scores scaled to a standard deviation of 1e-4 (ops.pca)")
    ap.add_argument("--pca", type=int, default=None, metavar="K",
                    help="the K leading principal components of the features on the device (ops.pca) and their explained variance")
    ap.add_argument("--pca_whiten", action="store_true", help="with --pca: scores of unit variance")
    ap.add_argument("--pca_out", type=str, default=None, metavar="PATH",
                    help="with --pca: write components, mean, explained_variance, explained_variance_ratio and scores as .npz")
    ap.add_argument("--norm", choices=["none", "both"], default="none",
                    help="none = the reference's plain in-edge sums; both = D^-1/2 A D^-1/2")
    ap.add_argument("--fused", choices=["auto", "on", "off"], default="auto",
                    help="on = the one-launch kernel or an error; off = batch -> encode -> readout in chunks of "
                         "--batch_size; auto = the kernel for every molecule it takes")
    ap.add_argument("--batch_size", "-b", type=int, default=4096, help="molecules per chunk of the chunked route")
    ap.add_argument("--seed", type=int, default=None, help="seed of --synthetic")
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
    if not args.out:
        parser.error("--out is required: the .npy file the features are written to")
    if bool(args.data_file) == bool(args.synthetic):
        parser.error("give exactly one of --data_file and --synthetic G")
    if args.synthetic < 0 or args.batch_size < 1 or args.in_dim < 1 or min(args.hidden_dims) < 1:
        parser.error("--synthetic, --batch_size, --in_dim and --hidden_dims take positive numbers")
    if args.fused == "on" and not ops.embed_graphs_usable(args.in_dim, args.hidden_dims, 0):
        parser.error(f"--fused on: the kernel takes 1..{ops.EMBED_MAX_LAYERS} layers of widths <= {ops.EMBED_MAX_WIDTH}, "
                     f"not {args.in_dim} -> {args.hidden_dims}; use --fused auto or off")
    if args.clusters is None:
        if args.clusters_out:
            parser.error("--clusters_out needs --clusters K")
    elif not 1 <= args.clusters <= 256 or 3 * args.hidden_dims[-1] > 64:
        parser.error(f"--clusters {args.clusters}: K must lie in 1..256 and the feature width 3 d = "
                     f"{3 * args.hidden_dims[-1]} must not exceed 64")
    if args.ridge is None:
        if args.ridge_out or args.ridge_folds is not None:
            parser.error("--ridge_out / --ridge_folds need --ridge")
    else:
        if not args.targets:
            parser.error("--ridge needs --targets PATH: the property (or properties) to regress on")
        if 3 * args.hidden_dims[-1] > ops.RIDGE_MAX_D:
            parser.error(f"--ridge: the feature width 3 d = {3 * args.hidden_dims[-1]} must not exceed {ops.RIDGE_MAX_D}")
        if args.ridge_folds is not None and not 2 <= args.ridge_folds <= ops.RIDGE_MAX_FOLDS:
            parser.error(f"--ridge_folds {args.ridge_folds}: F must lie in 2..{ops.RIDGE_MAX_FOLDS}")
        if len(args.ridge) > ops.RIDGE_MAX_LAMBDAS or not all(v >= 0.0 and v < float("inf") for v in args.ridge):
            parser.error(f"--ridge: at most {ops.RIDGE_MAX_LAMBDAS} finite values >= 0")
        if not os.path.exists(args.targets):
            parser.error(f"--targets {args.targets}: no such file")
    if args.forest is None:
        if args.forest_out or args.forest_depth is not None or args.forest_features is not None:
            parser.error("--forest_out / --forest_depth / --forest_features need --forest")
    else:
        if not args.targets:
            parser.error("--forest needs --targets PATH: the property (or properties) to regress on")
        if not 1 <= args.forest <= ops.FOREST_MAX_TREES or 3 * args.hidden_dims[-1] > ops.FOREST_MAX_D:
            parser.error(f"--forest {args.forest}: N_TREES must lie in 1..{ops.FOREST_MAX_TREES} and the feature width 3 d = "
                         f"{3 * args.hidden_dims[-1]} must not exceed {ops.FOREST_MAX_D}")
        if args.forest_depth is not None and not 1 <= args.forest_depth <= ops.FOREST_MAX_DEPTH:
            parser.error(f"--forest_depth {args.forest_depth}: D must lie in 1..{ops.FOREST_MAX_DEPTH}")
        if args.forest_features is not None and not 1 <= args.forest_features <= 3 * args.hidden_dims[-1]:
            parser.error(f"--forest_features {args.forest_features}: M must lie in 1..{3 * args.hidden_dims[-1]}")
        if not os.path.exists(args.targets):
            parser.error(f"--targets {args.targets}: no such file")
    if args.mlp is None:
        if args.mlp_out or any(v is not None for v in (args.mlp_epochs, args.mlp_batch, args.mlp_lr, args.mlp_alpha,
                                                        args.mlp_folds, args.mlp_ensemble)):
            parser.error("--mlp_out / --mlp_epochs / --mlp_batch / --mlp_lr / --mlp_alpha / --mlp_folds / --mlp_ensemble "
                         "need --mlp")
    else:
        if not args.targets:
            parser.error("--mlp needs --targets PATH: the property (or properties) to regress on")
        hidden = args.mlp or [100]
        if not 1 <= len(hidden) <= 2 or not all(1 <= h <= ops.MLP_MAX_WIDTH for h in hidden):
            parser.error(f"--mlp {' '.join(map(str, hidden))}: one or two hidden widths in 1..{ops.MLP_MAX_WIDTH}")
        if 3 * args.hidden_dims[-1] > ops.MLP_MAX_WIDTH:
            parser.error(f"--mlp: the feature width 3 d = {3 * args.hidden_dims[-1]} must not exceed {ops.MLP_MAX_WIDTH}")
        if (args.mlp_epochs is not None and args.mlp_epochs < 1) or (args.mlp_batch is not None and args.mlp_batch < 1) \
                or (args.mlp_ensemble is not None and args.mlp_ensemble < 1):
            parser.error("--mlp_epochs, --mlp_batch and --mlp_ensemble take positive numbers")
        if args.mlp_folds is not None and not 2 <= args.mlp_folds <= ops.MLP_MAX_FOLDS:
            parser.error(f"--mlp_folds {args.mlp_folds}: F must lie in 2..{ops.MLP_MAX_FOLDS}")
        if not all(0.0 < v < float("inf") for v in args.mlp_lr or []) \
                or not all(0.0 <= v < float("inf") for v in args.mlp_alpha or []):
            parser.error("--mlp_lr takes finite values > 0, --mlp_alpha finite values >= 0")
        models = ((args.mlp_folds or 5) + 1) * len(args.mlp_lr or [0]) * len(args.mlp_alpha or [0]) * (args.mlp_ensemble or 1)
        if models > ops.MLP_MAX_MODELS:
            parser.error(f"--mlp: (folds + 1) x learning rates x penalties x members = {models} models, at most "
                         f"{ops.MLP_MAX_MODELS} per call")
        if not os.path.exists(args.targets):
            parser.error(f"--targets {args.targets}: no such file")
    if args.logreg is None:
        if args.logreg_out or args.logreg_folds is not None or (args.labels and args.boost is None):
            parser.error("--logreg_out / --logreg_folds / --labels need --logreg (--labels: or --boost)")
    else:
        if not args.labels:
            parser.error("--logreg needs --labels PATH: the class of every molecule")
        if 3 * args.hidden_dims[-1] > ops.LOGREG_MAX_D:
            parser.error(f"--logreg: the feature width 3 d = {3 * args.hidden_dims[-1]} must not exceed {ops.LOGREG_MAX_D}")
        if args.logreg_folds is not None and not 2 <= args.logreg_folds <= ops.LOGREG_MAX_FOLDS:
            parser.error(f"--logreg_folds {args.logreg_folds}: F must lie in 2..{ops.LOGREG_MAX_FOLDS}")
        if len(args.logreg) > ops.LOGREG_MAX_LAMBDAS or not all(v >= 0.0 and v < float("inf") for v in args.logreg):
            parser.error(f"--logreg: at most {ops.LOGREG_MAX_LAMBDAS} finite values >= 0")
        if not os.path.exists(args.labels):
            parser.error(f"--labels {args.labels}: no such file")
    if args.boost is None:
        if args.boost_out or any(v is not None for v in (args.boost_depth, args.boost_lr, args.boost_lambda, args.boost_folds)):
            parser.error("--boost_out / --boost_depth / --boost_lr / --boost_lambda / --boost_folds need --boost")
    else:
        if not args.targets and not args.labels:
            parser.error("--boost needs --targets PATH (a property: the squared objective) or --labels PATH (classes 0 / 1: "
                         "the logistic objective)")
        if not 1 <= args.boost <= ops.BOOST_MAX_ROUNDS or 3 * args.hidden_dims[-1] > ops.BOOST_MAX_D:
            parser.error(f"--boost {args.boost}: N_ROUNDS must lie in 1..{ops.BOOST_MAX_ROUNDS} and the feature width 3 d = "
                         f"{3 * args.hidden_dims[-1]} must not exceed {ops.BOOST_MAX_D}")
        if args.boost_depth is not None and not 1 <= args.boost_depth <= ops.BOOST_MAX_DEPTH:
            parser.error(f"--boost_depth {args.boost_depth}: D must lie in 1..{ops.BOOST_MAX_DEPTH}")
        if args.boost_folds is not None and not 2 <= args.boost_folds <= 32:
            parser.error(f"--boost_folds {args.boost_folds}: F must lie in 2..32")
        if not all(0.0 < v <= 1.0 for v in args.boost_lr or []) \
                or not all(0.0 <= v < float("inf") for v in args.boost_lambda or []):
            parser.error("--boost_lr takes values in (0, 1], --boost_lambda finite values >= 0")
        models = ((args.boost_folds or 5) + 1) * len(args.boost_lr or [0]) * len(args.boost_lambda or [0])
        if models > ops.BOOST_MAX_MODELS:
            parser.error(f"--boost: (folds + 1) x learning rates x lambdas = {models} models, at most "
                         f"{ops.BOOST_MAX_MODELS} per call")
        for path in (args.targets, args.labels):
            if path and not os.path.exists(path):
                parser.error(f"{path}: no such file")
    if not args.map_out:
        if any(v is not None for v in (args.map_perplexity, args.map_iters, args.map_seed, args.map_init)):
            parser.error("--map_perplexity / --map_iters / --map_seed / --map_init need --map_out PATH")
    else:
        if args.map_init == "pca" and 3 * args.hidden_dims[-1] > ops.PCA_MAX_D:
            parser.error(f"--map_init pca: the feature width 3 d = {3 * args.hidden_dims[-1]} must not exceed {ops.PCA_MAX_D}")
        if 3 * args.hidden_dims[-1] > ops.KNN_MAX_D:
            parser.error(f"--map_out: the feature width 3 d = {3 * args.hidden_dims[-1]} must not exceed {ops.KNN_MAX_D}")
        if args.map_perplexity is not None and not 1.0 <= args.map_perplexity < 64.0:
            parser.error(f"--map_perplexity {args.map_perplexity}: P must lie in [1, 64)")
        if args.map_iters is not None and args.map_iters < 1:
            parser.error(f"--map_iters {args.map_iters}: T must be at least 1")
    if args.pca is None:
        if args.pca_whiten or args.pca_out:
            parser.error("--pca_whiten / --pca_out need --pca K")
    elif not 1 <= args.pca <= 3 * args.hidden_dims[-1] or 3 * args.hidden_dims[-1] > ops.PCA_MAX_D:
        parser.error(f"--pca {args.pca}: K must lie in 1..3 d = {3 * args.hidden_dims[-1]}, and 3 d must not exceed "
                     f"{ops.PCA_MAX_D}")
    if args.neighbours is None:
        if args.metric is not None or args.neighbours_out or (args.targets and args.ridge is None and args.forest is None
                                                              and args.mlp is None and args.boost is None):
            parser.error("--metric / --neighbours_out / --targets need --neighbours K (--targets: or --ridge / --forest / "
                         "--boost)")
    else:
        if not 1 <= args.neighbours <= ops.KNN_MAX_K or 3 * args.hidden_dims[-1] > ops.KNN_MAX_D:
            parser.error(f"--neighbours {args.neighbours}: K must lie in 1..{ops.KNN_MAX_K} and the feature width 3 d = "
                         f"{3 * args.hidden_dims[-1]} must not exceed {ops.KNN_MAX_D}")
        if args.targets and not os.path.exists(args.targets):
            parser.error(f"--targets {args.targets}: no such file")
    return args


def load_dataset(args, device):
    if args.synthetic:
        return DeviceGraphDataset.synthetic_zinc(args.synthetic, seed=args.seed or 0, device=device)
    if not os.path.exists(args.data_file):
        raise FileNotFoundError(f"{args.data_file} not found (use --synthetic G for ZINC-shaped synthetic data)")
    return DeviceGraphDataset.load(args.data_file, device=device)


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("gae_dgl_amd runs on AMD GPUs only (no CPU fallback)")
    device = torch.device(f"cuda:{args.gpu_id}")
    torch.cuda.set_device(device)
    model = GAE(args.in_dim, args.hidden_dims, norm=None if args.norm == "none" else args.norm)
    model.load_state_dict(torch.load(args.checkpoint, map_location="cpu"))
    model = model.to(device).eval()
    graphs = load_dataset(args, device)
    print(f"Loaded {len(graphs)} molecules")
    fused = {"auto": "auto", "on": True, "off": False}[args.fused]
    before = _lib.CALLS["gae_embed_graphs"]
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    feats = model.embed_graphs(graphs, fused=fused, batch_size=args.batch_size)
    torch.cuda.synchronize(device)
    seconds = time.perf_counter() - t0
    in_kernel = ops.embed_graphs.last_request["n_out"] if _lib.CALLS["gae_embed_graphs"] > before else 0
    route = "fused kernel" if in_kernel == len(graphs) else \
        "chunked route" if in_kernel == 0 else f"fused kernel for {in_kernel}, chunked route for {len(graphs) - in_kernel}"
    out = feats.cpu().numpy().astype(np.float32, copy=False)
    np.save(args.out, out)
    print(f"Embedded {out.shape[0]} molecules -> {tuple(out.shape)} fp32 | route: {route} | "
          f"{seconds * 1e3:.3f} ms | wrote {args.out}")
    main.features = feats
    main.scores = None
    if args.scores:
        from gae_dgl_amd import metrics
        sc = model.score_graphs(graphs, fused=fused, batch_size=args.batch_size)
        table = torch.stack([sc.loss.double(), sc.auc, sc.ap, sc.n_pos.double(), sc.n_neg.double()], 1).cpu().numpy()
        np.save(args.scores, table)
        summary = metrics.graph_score_summary(sc)
        print(f"Scored {table.shape[0]} molecules | AUC {summary['auc']:.4f} | AP {summary['ap']:.4f} | "
              f"loss (no dropout) {summary['loss']:.4f} | {summary['left_out']} without both classes | wrote {args.scores}")
        main.scores = sc
    main.clusters = None
    if args.clusters is not None:
        res = ops.kmeans(feats, args.clusters, seed=args.seed or 0)
        print(f"Clustered {out.shape[0]} molecules into {args.clusters} | inertia {res.inertia:.6g} | iterations: "
              f"{res.n_iter}{'' if res.converged else ' (not converged)'} | sizes: {res.counts.tolist()}")
        if args.clusters_out:
            np.savez(args.clusters_out, labels=res.labels.cpu().numpy(), centers=res.centers.cpu().numpy())
        main.clusters = res
    main.neighbours = None
    if args.neighbours is not None:
        from gae_dgl_amd import metrics
        metric = args.metric or "l2"
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        nn = ops.knn(feats, k=args.neighbours, metric=metric)
        torch.cuda.synchronize(device)
        print(f"Searched {out.shape[0]} molecules for their {args.neighbours} nearest ({metric}) | "
              f"{(time.perf_counter() - t0) * 1e3:.3f} ms (one call, set-up included)")
        main.neighbours = nn
        if args.neighbours_out:
            np.savez(args.neighbours_out, index=nn.index.cpu().numpy(), value=nn.value.cpu().numpy())
        if args.targets:
            y = np.load(args.targets)
            if y.shape[0] != out.shape[0] or (y.ndim > 1 and int(np.prod(y.shape[1:])) != 1):
                raise ValueError(f"--targets of shape {y.shape} for the kNN regressor on {out.shape[0]} molecules: one "
                                 f"property per molecule")
            y = torch.from_numpy(y.reshape(-1).astype(np.float64)).to(device)
            rm = metrics.regression_metrics(metrics.knn_predict(nn.index, nn.value, y), y)
            print(f"kNN ({args.neighbours}, leave-one-out) RMSE: {rm['rmse']:.6f} | MAE: {rm['mae']:.6f} | "
                  f"R2: {rm['r2']:.6f}")
            main.knn_scores = rm
    main.ridge = None
    if args.ridge is not None:
        y = np.load(args.targets)
        if y.ndim not in (1, 2) or y.shape[0] != out.shape[0]:
            raise ValueError(f"--targets of shape {y.shape} for {out.shape[0]} molecules: [G] or [G, t]")
        y = torch.from_numpy(y.astype(np.float32)).to(device)
        n_folds = args.ridge_folds or 5
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        res = ops.ridge(feats, y, args.ridge or None, folds=n_folds, seed=args.seed or 0)
        torch.cuda.synchronize(device)
        print(f"Fitted ridge on {res.n_used} molecules, {len(res.lambdas)} lambdas x {n_folds} folds | "
              f"{(time.perf_counter() - t0) * 1e3:.3f} ms (one call, set-up included)")
        chosen = res.lambdas.tolist().index(res.lam)
        pairs = " | ".join(f"RMSE: {r:.6f} | R2: {q:.6f}"
                           for r, q in zip(res.cv_rmse[chosen].tolist(), res.cv_r2[chosen].tolist()))
        print(f"Ridge ({n_folds}-fold CV, lambda = {res.lam:g}) {pairs}")
        if args.ridge_out:
            np.savez(args.ridge_out, coef=res.coef.cpu().numpy(), intercept=res.intercept.cpu().numpy(),
                     lam=np.float64(res.lam), lambdas=res.lambdas.cpu().numpy(), cv_rmse=res.cv_rmse.cpu().numpy(),
                     cv_r2=res.cv_r2.cpu().numpy())
        main.ridge = res
    main.forest = None
    if args.forest is not None:
        y = np.load(args.targets)
        if y.ndim not in (1, 2) or y.shape[0] != out.shape[0]:
            raise ValueError(f"--targets of shape {y.shape} for {out.shape[0]} molecules: [G] or [G, t]")
        y = torch.from_numpy(y.astype(np.float32)).to(device)
        depth = args.forest_depth or 12
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        res = ops.forest(feats, y, args.forest, max_depth=depth, max_features=args.forest_features or 1.0,
                         seed=args.seed or 0)
        torch.cuda.synchronize(device)
        print(f"Grew a forest on {res.n_used} molecules, {args.forest} trees of {int(res.n_nodes.sum())} nodes | "
              f"{(time.perf_counter() - t0) * 1e3:.3f} ms (one call, set-up included)")
        pairs = " | ".join(f"RMSE: {r:.6f} | R2: {q:.6f}" for r, q in zip(res.oob_rmse.tolist(), res.oob_r2.tolist()))
        print(f"Random Forest ({args.forest} trees, depth {depth}, out-of-bag) {pairs}")
        if args.forest_out:
            np.savez(args.forest_out, **{k: getattr(res, k).cpu().numpy() for k in (
                "feature", "threshold_bin", "threshold", "left", "count", "value", "gain", "n_nodes", "edges", "n_edges",
                "oob_prediction", "oob_rmse", "oob_r2", "importances")})
        main.forest = res
    main.mlp = None
    if args.mlp is not None:
        y = np.load(args.targets)
        if y.ndim not in (1, 2) or y.shape[0] != out.shape[0]:
            raise ValueError(f"--targets of shape {y.shape} for {out.shape[0]} molecules: [G] or [G, t]")
        y = torch.from_numpy(y.astype(np.float32)).to(device)
        hidden = tuple(args.mlp or [100])
        n_folds = args.mlp_folds or 5
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        res = ops.mlp(feats, y, hidden, lrs=args.mlp_lr or (1e-3,), alphas=args.mlp_alpha or (1e-4,),
                      epochs=args.mlp_epochs or 200, batch_size=args.mlp_batch or 200, folds=n_folds,
                      ensemble=args.mlp_ensemble or 1, seed=args.seed or 0)
        torch.cuda.synchronize(device)
        print(f"Trained an MLP head on {res.n_used} molecules, {res.info.numel()} models side by side | "
              f"{(time.perf_counter() - t0) * 1e3:.3f} ms (one call, set-up included)")
        chosen = res.lrs.index(res.lr) * len(res.alphas) + res.alphas.index(res.alpha)
        pairs = " | ".join(f"RMSE: {r:.6f} | R2: {q:.6f}"
                           for r, q in zip(res.cv_rmse[chosen].tolist(), res.cv_r2[chosen].tolist()))
        print(f"MLP ({' x '.join(map(str, hidden))}, {n_folds}-fold CV, lr = {res.lr:g}, alpha = {res.alpha:g}) {pairs}")
        if args.mlp_out:
            arrays = {"hidden": np.asarray(hidden, np.int64), "lr": np.float64(res.lr), "alpha": np.float64(res.alpha),
                      "shift": res.shift.cpu().numpy(), "scale": res.scale.cpu().numpy(),
                      "cv_rmse": res.cv_rmse.cpu().numpy(), "cv_r2": res.cv_r2.cpu().numpy()}
            for l, (W, b) in enumerate(zip(res.weights, res.biases)):
                arrays[f"weight{l}"] = W.cpu().numpy()
                arrays[f"bias{l}"] = b.cpu().numpy()
            np.savez(args.mlp_out, **arrays)
        main.mlp = res
    main.logreg = None
    if args.logreg is not None:
        from gae_dgl_amd import metrics
        from gae_dgl_amd.ops._heads import _default_fold
        y = np.load(args.labels)
        if y.ndim != 1 or y.shape[0] != out.shape[0] or not np.issubdtype(y.dtype, np.integer):
            raise ValueError(f"--labels of shape {y.shape}, {y.dtype} for {out.shape[0]} molecules: integer classes [G]")
        y = torch.from_numpy(y.astype(np.int64)).to(device)
        n_folds = args.logreg_folds or 5
        fold = _default_fold(out.shape[0], n_folds, args.seed or 0).to(device)
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        res = ops.logreg(feats, y, args.logreg or None, folds=n_folds, fold=fold)
        torch.cuda.synchronize(device)
        print(f"Fitted logistic regression on {res.n_used} molecules, {res.coef.shape[0]} classes, {len(res.lambdas)} lambdas x "
              f"{n_folds} folds | passes: {int(res.n_iter.max())} at most"
              f"{'' if bool(res.converged.all()) else ' (not all converged)'} | "
              f"{(time.perf_counter() - t0) * 1e3:.3f} ms (one call, set-up included)")
        chosen = res.lambdas.tolist().index(res.lam)
        c = res.coef.shape[0]
        pred = torch.full((out.shape[0],), -1, dtype=torch.int32, device=device)
        proba = torch.full((out.shape[0], c), float("nan"), dtype=torch.float32, device=device)
        for f in range(n_folds):                                       # every labelled molecule by the model that did not see it
            idx = ((fold == f) & (y >= 0)).nonzero().reshape(-1)
            pf, qf = ops.logreg_predict(feats.index_select(0, idx).contiguous(), res.fold_coef[f, chosen],
                                        res.fold_intercept[f, chosen], res.pivot, proba=True)
            pred[idx], proba[idx] = pf, qf
        cm = metrics.classification_metrics(pred, y, proba, n_classes=c)
        print(f"LogReg ({n_folds}-fold CV, lambda = {res.lam:g}) accuracy: {cm['accuracy']:.4f} | "
              f"macro-F1: {cm['macro_f1']:.4f} | log-loss: {cm['log_loss']:.4f}")
        if args.logreg_out:
            np.savez(args.logreg_out, coef=res.coef.cpu().numpy(), intercept=res.intercept.cpu().numpy(),
                     pivot=res.pivot.cpu().numpy(), lam=np.float64(res.lam), lambdas=res.lambdas.cpu().numpy(),
                     cv_logloss=res.cv_logloss.cpu().numpy(), cv_accuracy=res.cv_accuracy.cpu().numpy())
        main.logreg = res
        main.logreg_scores = cm
    main.boost = None
    if args.boost is not None:
        from gae_dgl_amd import metrics
        depth, n_folds = args.boost_depth or 4, args.boost_folds or 5
        lrs, lams = tuple(args.boost_lr or (0.1,)), tuple(args.boost_lambda or (1.0,))
        runs = []
        if args.targets:
            y = np.load(args.targets)
            if y.shape[0] != out.shape[0] or (y.ndim > 1 and int(np.prod(y.shape[1:])) != 1):
                raise ValueError(f"--targets of shape {y.shape} for --boost on {out.shape[0]} molecules: one property per "
                                 f"molecule")
            runs.append(("squared", torch.from_numpy(y.reshape(-1).astype(np.float32)).to(device)))
        if args.labels:
            y = np.load(args.labels)
            if y.ndim != 1 or y.shape[0] != out.shape[0] or not np.issubdtype(y.dtype, np.integer):
                raise ValueError(f"--labels of shape {y.shape}, {y.dtype} for {out.shape[0]} molecules: integer classes [G]")
            runs.append(("logistic", torch.from_numpy(y.astype(np.int64)).to(device)))
        main.boost_scores = {}
        for objective, y in runs:
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            res = ops.boost(feats, y, objective, args.boost, max_depth=depth, learning_rates=lrs, lambdas=lams, folds=n_folds,
                            seed=args.seed or 0, oof=True)
            torch.cuda.synchronize(device)
            print(f"Boosted {objective} trees on {res.n_used} molecules, {(n_folds + 1) * len(lrs) * len(lams)} models side by "
                  f"side | {(time.perf_counter() - t0) * 1e3:.3f} ms (two calls, set-up included)")
            head = f"Boosting ({res.best_round} of {args.boost} rounds, depth {depth}, {n_folds}-fold CV, lr = {res.lr:g}, " \
                   f"lambda = {res.lam:g})"
            if objective == "squared":
                sc = metrics.regression_metrics(res.oof_score, y.double())
                print(f"{head} RMSE: {sc['rmse']:.6f} | R2: {sc['r2']:.6f}")
            else:
                keep = y >= 0
                p1 = torch.sigmoid(res.oof_score)
                proba = torch.stack([1.0 - p1, p1], 1)
                sc = metrics.classification_metrics((res.oof_score >= 0).to(torch.int32), y[keep], proba, n_classes=2)
                print(f"{head} accuracy: {sc['accuracy']:.4f} | ROC-AUC: {sc['roc_auc']:.4f} | log-loss: {sc['log_loss']:.4f}")
            main.boost_scores[objective] = sc
            main.boost = res
        if args.boost_out:
            np.savez(args.boost_out, base_score=np.float64(res.base_score), lr=np.float64(res.lr), lam=np.float64(res.lam),
                     best_round=np.int64(res.best_round), **{k: getattr(res, k).cpu().numpy() for k in (
                         "feature", "threshold_bin", "threshold", "left", "count", "value", "gain", "n_nodes", "edges",
                         "n_edges", "cv_curve", "importances")})
    main.pca = None
    if args.pca is not None:
        res = ops.pca(feats, args.pca, whiten=args.pca_whiten)
        ratio = res.explained_variance_ratio.cpu().numpy()
        print(f"PCA ({args.pca} of {out.shape[1]} components) explained variance: "
              f"{' '.join(f'{v:.4f}' for v in ratio)} (cumulative {float(ratio.sum()):.4f})")
        if args.pca_out:
            np.savez(args.pca_out, components=res.components.cpu().numpy(), mean=res.mean.cpu().numpy(),
                     explained_variance=res.explained_variance.cpu().numpy(), explained_variance_ratio=ratio,
                     scores=res.transform(feats).cpu().numpy())
        main.pca = res
    main.map = None
    if args.map_out:
        from gae_dgl_amd import metrics
        P = 20.0 if args.map_perplexity is None else args.map_perplexity
        res = ops.tsne(feats, perplexity=P, n_iter=1000 if args.map_iters is None else args.map_iters,
                       seed=args.map_seed or 0, init="pca" if args.map_init == "pca" else None)
        k10 = min(10, out.shape[0] - 1)
        keep = metrics.neighbourhood_preservation(ops.knn(feats, k=k10).index, ops.knn(res.embedding, k=k10).index)
        print(f"t-SNE (perplexity {P:g}, {res.n_iter} iterations) KL: {res.kl_divergence:.4f} | "
              f"10-NN preservation: {keep:.4f}")
        labels = np.load(args.labels).astype(np.int64).reshape(-1) if args.labels else np.full(out.shape[0], -1, np.int64)
        np.savez(args.map_out, embedding=res.embedding.cpu().numpy(), labels=labels, kl_divergence=res.kl_divergence,
                 kl_curve=np.asarray(res.kl_curve, np.float64).reshape(-1, 2))
        main.map = res
        main.map_preservation = keep
    return out


if __name__ == '__main__':
    main()
