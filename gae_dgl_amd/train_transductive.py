"""Counterpart of gae_dgl/train_transductive.py (which cannot run as written,
README.md:19): full-graph GAE training on a citation graph, reproducing the
file's INTENT -- ``GAE(in_feats, [32, 16])``, Adam lr 1e-2, 500 full-graph
epochs, ``pos_weight`` from the dense label (train_transductive.py:41,43,49,
59-60) -- on the HIP kernels.

  python -m gae_dgl_amd.train_transductive --dataset cora [--norm both] [--eval [--rank]] [--topk 10 [--topk_out top.npz]]
      [--loss_samples M] [--decode_out graph.npz [--decode_prob P] [--decode_max_pairs M]]
      [--cluster K [--cluster_seed S] [--cluster_out clusters.npz]] [--knn K [--knn_metric l2|dot|cosine]]
      [--classify [LAMBDA ...] [--classify_folds F] [--classify_test_frac Q] [--classify_seed S] [--classify_out model.npz]]
      [--map_out map.npz [--map_perplexity P] [--map_iters T] [--map_seed S] [--map_init random|pca]]
      [--pca K [--pca_out pca.npz]]
      [--spectral K [--spectral_self_loops] [--spectral_scaling none|degree|value] [--spectral_seed N] [--spectral_out sc.npz]]
      [--heuristics [cn|jaccard|aa|ra|pa ...] [--heuristics_out pairs.npz]]
      [--deepwalk D [--deepwalk_walks R] [--deepwalk_length L] [--deepwalk_window W] [--deepwalk_epochs E] [--deepwalk_seed S]
       [--deepwalk_out dw.npz]]

``--norm both`` applies the ``deg^-1/2`` normalisation the reference computes
at :55-58 but never feeds to the model (north-star D^-1/2 A D^-1/2); the
default ``none`` is the reference's actual arithmetic."""
import argparse
import os

import torch

from gae_dgl_amd import DGLGraph
from gae_dgl_amd.data import load_data, register_data_args
from gae_dgl_amd.gae import GAE

HEURISTIC_KINDS = ("cn", "jaccard", "aa", "ra", "pa")


def build_parser():
    ap = argparse.ArgumentParser(description="Pre-train GAE")
    register_data_args(ap)                                       # --dataset, as dgl.data.register_data_args
    # the reference's flags (train_transductive.py:18-27); it ignores most of them and hard-codes [32, 16],
    # lr 1e-2 and 500 epochs (:41,43,49), which are the defaults here
    for names, kind, default, text in (
            (("--n_epochs", "-e"), int, 500, "full-graph epochs"),
            (("--save_dir", "-s"), str, "../result", "where the checkpoint goes"),
            (("--in_dim", "-i"), int, 39, "ignored: the width comes from the data"),
            (("--batch_size", "-b"), int, 128, "unused (full graph)"),
            (("--lr",), float, 1e-2, "Adam step size"),
            (("--gpu_id",), int, 0, "which GPU")):
        ap.add_argument(*names, type=kind, default=default, help=text)
    ap.add_argument("--hidden_dims", type=int, nargs="+", metavar="N", default=[32, 16], help="encoder widths")
    # extensions
    ap.add_argument("--norm", choices=["none", "both"], default="none")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--log_every", type=int, default=50)
    ap.add_argument("--features", choices=["auto", "dense"], default="auto",
                    help="auto: the features are loaded once and stay constant (the reference's train_transductive.py:37-38), "
                         "so they are compressed at load time WHERE layer 1 runs faster from their non-zeros "
                         "(SparseFeatures.maybe_from_dense: Citeseer, Cora); dense: always the dense FloatTensor")
    ap.add_argument("--no_hipgraph", action="store_true",
                    help="launch every kernel from Python instead of replaying the captured step")
    ap.add_argument("--eval", action="store_true",
                    help="hold out 5 %% / 10 %% of the edges (the reference's '# TODO: train test split', :35) and "
                         "report link-prediction ROC-AUC / AP on them after training")
    ap.add_argument("--topk", type=int, default=None, metavar="K",
                    help="after training, the K (1..64) most likely new neighbours of every node (GAE.predict_links, "
                         "known edges left out); with --eval prints the test recall@K, with --topk_out saves them")
    ap.add_argument("--topk_out", default=None, metavar="PATH",
                    help="write the --topk lists to PATH (.npz with 'index' int64 [n, K] and 'score' fp32 [n, K])")
    ap.add_argument("--rank", action="store_true",
                    help="with --eval: rank both directions of every held-out test pair among ALL candidates of its "
                         "source (GAE.rank_links, every edge of the input graph filtered) and print the test MRR, "
                         "Hits@10 / @100, mean rank and the all-non-edges AUC")
    ap.add_argument("--loss_samples", type=int, default=None, metavar="M",
                    help="train on the unbiased sampled loss (GAE.reconstruction_loss(g, samples=M)): the edge term "
                         "exactly, the all-pairs term from M random partners per node, O((E + N M) d) per step")
    ap.add_argument("--decode_out", default=None, metavar="PATH",
                    help="after training, decode the training graph (GAE.reconstruct: the pairs with sigmoid(z_i . z_j) "
                         ">= P, no N x N matrix), print its precision / recall / F1 against the graph and write the CSR "
                         "to PATH (.npz with 'indptr' int64 [n + 1], 'index' int32 [nnz], 'score' fp32 [nnz])")
    ap.add_argument("--decode_prob", type=float, default=None, metavar="P",
                    help="with --decode_out: the probability cut-off, inside (0, 1) (default 0.5)")
    ap.add_argument("--decode_max_pairs", type=int, default=None, metavar="M",
                    help="with --decode_out: refuse to write more than M pairs (default 2^27, 12 bytes each)")
    ap.add_argument("--cluster", type=int, default=None, metavar="K",
                    help="after training, k-means with K (1..256) clusters on the node embedding (GAE.cluster_nodes, on "
                         "the device): prints the inertia, the iterations and the cluster sizes, and NMI | ARI | ACC "
                         "where the dataset carries class labels")
    ap.add_argument("--cluster_seed", type=int, default=None, metavar="S",
                    help="with --cluster: the seed of the k-means++ seeding (default 0)")
    ap.add_argument("--cluster_out", default=None, metavar="PATH",
                    help="with --cluster: write PATH (.npz with 'labels' int32 [n] and 'centers' fp32 [K, d])")
    ap.add_argument("--knn", type=int, default=None, metavar="K",
                    help="after training, the leave-one-out kNN accuracy of the node embedding against the class labels: "
                         "every labelled node takes the plurality class of its K (1..64) nearest "
                         "neighbours (GAE.nearest_nodes, on the device); unlabelled nodes neither vote nor are scored")
    ap.add_argument("--knn_metric", choices=["l2", "dot", "cosine"], default=None,
                    help="with --knn: squared Euclidean distance (default), inner product or cosine similarity")
    ap.add_argument("--classify", type=float, nargs="*", default=None, metavar="LAMBDA",
                    help="after training, the standard protocol for the frozen node embedding: a seeded split of the "
                         "labelled nodes, multinomial logistic regression on the training part with the penalty chosen "
                         "by F-fold CV among the LAMBDAs (default 10^-3 .. 10^3, 13 values) on the device "
                         "(GAE.classify_nodes), then accuracy | macro-F1 | log-loss on the test part")
    ap.add_argument("--classify_folds", type=int, default=None, metavar="F", help="with --classify: CV folds, 2..32 (default 5)")
    ap.add_argument("--classify_test_frac", type=float, default=None, metavar="Q",
                    help="with --classify: the share of the labelled nodes kept out as the test part, inside (0, 1) "
                         "(default 0.2)")
    ap.add_argument("--classify_seed", type=int, default=None, metavar="S",
                    help="with --classify: the seed of the split and of the folds (default 0)")
    ap.add_argument("--classify_out", default=None, metavar="PATH",
                    help="with --classify: write PATH (.npz with 'coef' fp64 [c, d], 'intercept' [c], 'lam', 'lambdas', "
                         "'cv_logloss', 'cv_accuracy', 'test_index' int64 and 'test_pred' int32)")
    ap.add_argument("--map_out", default=None, metavar="PATH",
                    help="after training: the 2-D map of the embedding by exact t-SNE on the device (GAE.map_nodes) and its "
                         "10-NN preservation; writes PATH (.npz with 'embedding' fp32 [N, 2], 'labels' int64 [N] (-1 where "
                         "the dataset has none), 'kl_divergence' and 'kl_curve')")
    ap.add_argument("--map_perplexity", type=float, default=None, metavar="P",
                    help="with --map_out: the perplexity, at least 1 and below min(N - 1, 64) (default 20)")
    ap.add_argument("--map_iters", type=int, default=None, metavar="T", help="with --map_out: iterations (default 1000)")
    ap.add_argument("--map_seed", type=int, default=None, metavar="S", help="with --map_out: the seed of the start (default 0)")
    ap.add_argument("--map_init", choices=["random", "pca"], default=None,
                    help="with --map_out: the start of the map, the library's Philox draw (default) or the first two principal "
                         "scores scaled to a standard deviation of 1e-4 (ops.pca)")
    ap.add_argument("--pca", type=int, default=None, metavar="K",
                    help="after training: the K leading principal components of the node embedding on the device "
                         "(GAE.pca_nodes) and their explained variance")
    ap.add_argument("--pca_out", default=None, metavar="PATH",
                    help="with --pca: write PATH (.npz with 'components' fp64 [K, d], 'mean', 'explained_variance', "
                         "'explained_variance_ratio' and 'scores' fp32 [N, K])")
    ap.add_argument("--spectral", type=int, default=None, metavar="K",
                    help="with --eval: the spectral-clustering baseline of the GAE tables -- the K leading eigenvectors of "
                         "the normalised adjacency of the TRAINING graph (ops.spectral_embedding), scored like the "
                         "model's embedding; with --cluster / --classify the same k-means and log-reg lines for it")
    ap.add_argument("--spectral_self_loops", action="store_true", help="with --spectral: the GCN operator (A + I)")
    ap.add_argument("--spectral_scaling", choices=["none", "degree", "value"], default=None,
                    help="with --spectral: the scaling of the embedding (default none)")
    ap.add_argument("--spectral_seed", type=int, default=None, metavar="N", help="with --spectral: the seed of the start block (default 0)")
    ap.add_argument("--spectral_out", default=None, metavar="PATH",
                    help="with --spectral: write PATH (.npz with 'embedding' fp32 [N, K], 'vectors' fp64, 'values', 'residuals')")
    ap.add_argument("--heuristics", nargs="*", choices=HEURISTIC_KINDS, default=None, metavar="KIND",
                    help="with --eval: the neighbourhood baselines of a link-prediction table -- common neighbours (cn), "
                         "jaccard, Adamic-Adar (aa), resource allocation (ra), preferential attachment (pa); no KIND: all "
                         "five -- of the val / test pairs on the TRAINING graph (ops.neighbour_scores), ROC-AUC | AP beside "
                         "the model's lines; with --topk K also their test recall@K (ops.neighbour_topk; not for pa)")
    ap.add_argument("--heuristics_out", default=None, metavar="PATH",
                    help="with --heuristics: write the per-pair tables to PATH (.npz: '{val,test}_{pos,neg}_pairs' int64 "
                         "[2, m] and '{val,test}_{pos,neg}_KIND' for common, deg_i, deg_j and every KIND)")
    ap.add_argument("--deepwalk", type=int, default=None, metavar="D",
                    help="with --eval: the DeepWalk baseline of the GAE tables -- a D-wide skip-gram embedding of random walks "
                         "over the TRAINING graph (ops.deepwalk: synchronous mini-batch Adagrad with shared negatives, "
                         "DeepWalk-like), scored like the model's embedding; with --cluster / --classify the same k-means and "
                         "log-reg lines for it")
    ap.add_argument("--deepwalk_walks", type=int, default=None, metavar="R", help="with --deepwalk: walks per node (default 10)")
    ap.add_argument("--deepwalk_length", type=int, default=None, metavar="L", help="with --deepwalk: nodes per walk, 2..64 (default 40)")
    ap.add_argument("--deepwalk_window", type=int, default=None, metavar="W",
                    help="with --deepwalk: the skip-gram window, 1..L - 1 (default 5)")
    ap.add_argument("--deepwalk_epochs", type=int, default=None, metavar="E", help="with --deepwalk: passes over the walks (default 3)")
    ap.add_argument("--deepwalk_seed", type=int, default=None, metavar="S", help="with --deepwalk: the seed of the walks, the "
                    "start table, the walk order and the negatives (default 0)")
    ap.add_argument("--deepwalk_out", default=None, metavar="PATH",
                    help="with --deepwalk: write PATH (.npz with 'embedding' and 'context' fp32 [N, D], 'walks' int32 and 'counts')")
    return ap


def parse_args(argv=None):
    """the parsed flags; combinations that cannot run are refused here, before any device is touched"""
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.topk is not None:
        if not 1 <= args.topk <= 64:
            ap.error(f"--topk {args.topk}: K must lie in 1..64")
        if not args.eval and args.topk_out is None:
            ap.error("--topk needs --eval (recall@K on the held-out edges) or --topk_out PATH")
    elif args.topk_out is not None:
        ap.error("--topk_out needs --topk K")
    if args.rank and not args.eval:
        ap.error("--rank needs --eval (it ranks the held-out test edges)")
    if args.loss_samples is not None and args.loss_samples < 1:
        ap.error(f"--loss_samples {args.loss_samples}: M must be at least 1")
    if args.decode_out is None:
        if args.decode_prob is not None or args.decode_max_pairs is not None:
            ap.error("--decode_prob / --decode_max_pairs need --decode_out PATH")
    else:
        if args.decode_prob is not None and not 0.0 < args.decode_prob < 1.0:
            ap.error(f"--decode_prob {args.decode_prob}: P must lie inside (0, 1)")
        if args.decode_max_pairs is not None and args.decode_max_pairs < 1:
            ap.error(f"--decode_max_pairs {args.decode_max_pairs}: M must be at least 1")
    if args.cluster is None:
        if args.cluster_seed is not None or args.cluster_out is not None:
            ap.error("--cluster_seed / --cluster_out need --cluster K")
    elif not 1 <= args.cluster <= 256:
        ap.error(f"--cluster {args.cluster}: K must lie in 1..256")
    if args.knn is None:
        if args.knn_metric is not None:
            ap.error("--knn_metric needs --knn K")
    elif not 1 <= args.knn <= 64:
        ap.error(f"--knn {args.knn}: K must lie in 1..64")
    if args.classify is None:
        if any(v is not None for v in (args.classify_folds, args.classify_test_frac, args.classify_seed, args.classify_out)):
            ap.error("--classify_folds / --classify_test_frac / --classify_seed / --classify_out need --classify")
    else:
        if len(args.classify) > 64:
            ap.error(f"--classify: at most 64 LAMBDAs, not {len(args.classify)}")
        if not all(v >= 0.0 and v < float("inf") for v in args.classify):
            ap.error(f"--classify {args.classify}: finite values >= 0")
        if args.classify_folds is not None and not 2 <= args.classify_folds <= 32:
            ap.error(f"--classify_folds {args.classify_folds}: F must lie in 2..32")
        if args.classify_test_frac is not None and not 0.0 < args.classify_test_frac < 1.0:
            ap.error(f"--classify_test_frac {args.classify_test_frac}: Q must lie inside (0, 1)")
    if args.map_out is None:
        if any(v is not None for v in (args.map_perplexity, args.map_iters, args.map_seed, args.map_init)):
            ap.error("--map_perplexity / --map_iters / --map_seed / --map_init need --map_out PATH")
    else:
        if args.map_perplexity is not None and not 1.0 <= args.map_perplexity < 64.0:
            ap.error(f"--map_perplexity {args.map_perplexity}: P must lie in [1, 64)")
        if args.map_iters is not None and args.map_iters < 1:
            ap.error(f"--map_iters {args.map_iters}: T must be at least 1")
    if args.pca is None:
        if args.pca_out is not None:
            ap.error("--pca_out needs --pca K")
    elif not 1 <= args.pca <= args.hidden_dims[-1] or args.hidden_dims[-1] > 128:
        ap.error(f"--pca {args.pca}: K must lie in 1..{args.hidden_dims[-1]} (the embedding width, 128 at the most)")
    if args.spectral is None:
        if args.spectral_self_loops or any(v is not None for v in (args.spectral_scaling, args.spectral_seed, args.spectral_out)):
            ap.error("--spectral_self_loops / --spectral_scaling / --spectral_seed / --spectral_out need --spectral K")
    else:
        if not 1 <= args.spectral <= 64:
            ap.error(f"--spectral {args.spectral}: K must lie in 1..64")
        if not args.eval:
            ap.error("--spectral needs --eval (it scores the held-out edges)")
        if args.spectral_seed is not None and args.spectral_seed < 0:
            ap.error(f"--spectral_seed {args.spectral_seed}: N must be at least 0")
    if args.heuristics is None:
        if args.heuristics_out is not None:
            ap.error("--heuristics_out needs --heuristics")
    elif not args.eval:
        ap.error("--heuristics needs --eval (it scores the held-out edges)")
    if args.deepwalk is None:
        if any(v is not None for v in (args.deepwalk_walks, args.deepwalk_length, args.deepwalk_window, args.deepwalk_epochs,
                                       args.deepwalk_seed, args.deepwalk_out)):
            ap.error("--deepwalk_walks / --deepwalk_length / --deepwalk_window / --deepwalk_epochs / --deepwalk_seed / "
                     "--deepwalk_out need --deepwalk D")
    else:
        if not 1 <= args.deepwalk <= 128:
            ap.error(f"--deepwalk {args.deepwalk}: D must lie in 1..128")
        if not args.eval:
            ap.error("--deepwalk needs --eval (it scores the held-out edges)")
        if args.deepwalk_walks is not None and args.deepwalk_walks < 1:
            ap.error(f"--deepwalk_walks {args.deepwalk_walks}: R must be at least 1")
        length = 40 if args.deepwalk_length is None else args.deepwalk_length
        if not 2 <= length <= 64:
            ap.error(f"--deepwalk_length {length}: L must lie in 2..64")
        window = 5 if args.deepwalk_window is None else args.deepwalk_window
        if not 1 <= window < length:
            ap.error(f"--deepwalk_window {window}: W must lie in 1..L - 1 = {length - 1}")
        if args.deepwalk_epochs is not None and args.deepwalk_epochs < 1:
            ap.error(f"--deepwalk_epochs {args.deepwalk_epochs}: E must be at least 1")
        if args.deepwalk_seed is not None and args.deepwalk_seed < 0:
            ap.error(f"--deepwalk_seed {args.deepwalk_seed}: S must be at least 0")
    return args


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("gae_dgl_amd runs on AMD GPUs only (no CPU fallback)")
    device = torch.device(f"cuda:{args.gpu_id}")
    torch.cuda.set_device(device)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    os.makedirs(args.save_dir, exist_ok=True)

    from gae_dgl_amd import metrics, ops
    from gae_dgl_amd.capture import CapturedTrainStep
    from gae_dgl_amd.optim import Adam
    data = load_data(args)
    features = ops.pad_rows(torch.as_tensor(data.features, dtype=torch.float32).to(device))   # 16 / 128-byte rows
    n_nodes = data.graph.number_of_nodes()
    held_out = None
    if args.eval:
        src, dst = (data.graph.src, data.graph.dst) if hasattr(data.graph, "src") else \
            tuple(map(list, zip(*data.graph.edges())))
        kept, val, test = metrics.split_edges(src, dst, n_nodes, seed=args.seed or 0)
        held_out = {"val": val, "test": test}
        g = DGLGraph(kept, num_nodes=n_nodes).to(device)
    else:
        g = DGLGraph(data.graph).to(device)
    g.ndata['norm'] = g.norm().unsqueeze(1)    # train_transductive.py:55-58; parameter independent: once, not per epoch
    if args.features == "auto" and device.type == "cuda":
        # decided per GRAPH: the kernels on the non-zeros need a table-only plan, which every graph whose longest row
        # has <= ops.TABLE_MAX_ROW (1024) edges gets -- real Cora / Citeseer (hubs of 168 / 99 neighbours) qualify
        from gae_dgl_amd import SparseFeatures
        features = SparseFeatures.maybe_from_dense(features, args.hidden_dims[0], graph=g)

    model = GAE(features.shape[1], args.hidden_dims, norm=args.norm).to(device).train()
    optimiser = Adam(model.parameters(), lr=args.lr)      # torch.optim.Adam's rule, one HIP launch

    def eager_step():
        g.ndata['h'] = features
        loss = model.reconstruction_loss(g, samples=args.loss_samples)
        optimiser.zero_grad()
        ops.backward(loss)                # loss.backward() with a cached unit gradient
        optimiser.step()
        return loss.detach()

    # The step is a fixed sequence of ~25 launches on static buffers: after the first epoch (which creates the
    # optimiser state and every cached workspace) it is captured once and replayed as one HIP graph.
    step = eager_step
    losses = []
    print("Training Start")
    for epoch in range(args.n_epochs):
        if epoch == 1 and not args.no_hipgraph:
            step = CapturedTrainStep(model, optimiser, g, features, warmup=0) if args.loss_samples is None else \
                CapturedTrainStep(model, optimiser, g, features, warmup=0,
                                  loss_fn=lambda m, gr: m.reconstruction_loss(gr, samples=args.loss_samples))
        losses.append(step().clone())
        if epoch % args.log_every == 0 or epoch + 1 == args.n_epochs:
            print(f"Epoch: {epoch:02d} | Loss: {float(losses[-1]):.5f}")
    torch.save(model.state_dict(), os.path.join(args.save_dir, f"transductive_{args.dataset}.pkl"))
    if held_out is not None:
        g.ndata['h'] = features
        with torch.no_grad():
            Z = model.encode(g)
        for name, pairs in held_out.items():
            scores = metrics.evaluate(Z, pairs)
            print(f"{name} ROC-AUC: {scores['auc']:.4f} | AP: {scores['ap']:.4f}")
        main.last_eval = metrics.evaluate(Z, held_out["test"])
    if args.rank:
        # filtered protocol: train, validation and test edges are all left out of the candidates; the target of a query
        # is exempt from the filter (gae_decoder_rank), so every held-out test edge still gets its rank
        import numpy as np
        pos = held_out["test"]["pos"]
        queries = np.concatenate([pos, pos[::-1]], axis=1)
        every = [np.concatenate([np.asarray(kept[k], dtype=np.int64), held_out["val"]["pos"][k],
                                 held_out["val"]["pos"][1 - k], pos[k], pos[1 - k]]) for k in (0, 1)]
        full = DGLGraph((every[0], every[1]), num_nodes=n_nodes).to(device)
        g.ndata['h'] = features
        res = model.rank_links(g, queries, filter_graph=full)
        rm = metrics.rank_metrics(res.greater, res.equal, res.candidates, ks=(1, 10, 50, 100))
        print(f"test MRR: {rm['mrr']:.4f} | Hits@10: {rm['hits@10']:.4f} | Hits@100: {rm['hits@100']:.4f} | "
              f"mean rank: {rm['mean_rank']:.1f} | AUC (all non-edges): {rm['auc']:.4f}")
        main.last_rank = rm
    if args.topk is not None:
        # the training graph's edges are left out, so the held-out test positives are candidates
        g.ndata['h'] = features
        score, index = model.predict_links(g, args.topk)
        if held_out is not None:
            recall = metrics.recall_at_k(index, held_out["test"]["pos"])
            print(f"test recall@{args.topk}: {recall:.4f}")
            main.last_recall = recall
        if args.topk_out is not None:
            import numpy as np
            np.savez(args.topk_out, index=index.cpu().numpy(), score=score.cpu().numpy())
    if args.decode_out is not None:
        import numpy as np
        g.ndata['h'] = features
        links = model.reconstruct(g, prob=0.5 if args.decode_prob is None else args.decode_prob,
                                  max_pairs=2 ** 27 if args.decode_max_pairs is None else args.decode_max_pairs)
        rm = metrics.reconstruction_metrics(links.indptr, links.index, *g.csr())
        print(f"reconstruction precision: {rm['precision']:.4f} | recall: {rm['recall']:.4f} | F1: {rm['f1']:.4f} | "
              f"predicted pairs: {rm['n_pred']}")
        main.last_decode = rm
        np.savez(args.decode_out, indptr=links.indptr.cpu().numpy(), index=links.index.cpu().numpy(),
                 score=links.score.cpu().numpy())
    if args.cluster is not None:
        import numpy as np
        g.ndata['h'] = features
        res = model.cluster_nodes(g, args.cluster, seed=args.cluster_seed or 0)
        print(f"k-means K = {args.cluster}: inertia {res.inertia:.6g} | iterations: {res.n_iter}"
              f"{'' if res.converged else ' (not converged)'} | sizes: {res.counts.tolist()}")
        main.last_cluster = {"result": res}
        if data.labels is not None:
            cm = metrics.clustering_metrics(res.labels.cpu().numpy(), data.labels)
            print(f"NMI: {cm['nmi']:.4f} | ARI: {cm['ari']:.4f} | ACC: {cm['acc']:.4f}")
            main.last_cluster.update(cm)
        if args.cluster_out is not None:
            np.savez(args.cluster_out, labels=res.labels.cpu().numpy(), centers=res.centers.cpu().numpy())
    if args.knn is not None:
        main.last_knn = None
        if data.labels is None:
            print(f"kNN K = {args.knn}: the dataset carries no class labels, nothing to score")
        else:
            g.ndata['h'] = features
            nn = model.nearest_nodes(g, args.knn, metric=args.knn_metric or "l2")
            labels = torch.as_tensor(data.labels, dtype=torch.int64, device=device)
            pred = metrics.knn_predict(nn.index, nn.value, labels, task="classification")
            scored = (labels >= 0) & (pred >= 0)
            acc = float((pred[scored] == labels[scored]).double().mean()) if bool(scored.any()) else float("nan")
            print(f"kNN K = {args.knn} ({args.knn_metric or 'l2'}, leave-one-out) accuracy: {acc:.4f} | "
                  f"nodes scored: {int(scored.sum())} of {n_nodes}")
            main.last_knn = {"acc": acc, "n": int(scored.sum()), "result": nn, "pred": pred, "model": model, "graph": g,
                             "features": features}
    if args.classify is not None:
        import numpy as np
        main.last_classify = None
        if data.labels is None:
            print("LogReg: the dataset carries no class labels, nothing to fit")
        else:
            F = args.classify_folds or 5
            labels = torch.as_tensor(data.labels, dtype=torch.int64, device=device)
            known = (labels >= 0).nonzero().reshape(-1).cpu()
            gen = torch.Generator(device="cpu").manual_seed(args.classify_seed or 0)
            perm = known[torch.randperm(known.numel(), generator=gen)]
            n_test = max(1, int(round((0.2 if args.classify_test_frac is None else args.classify_test_frac) * perm.numel())))
            test, train = perm[:n_test], perm[n_test:]
            fold = torch.full((n_nodes,), -1, dtype=torch.int64)
            fold[train] = torch.arange(train.numel()) % F               # the test part enters as fold = -1: never read
            g.ndata['h'] = features
            res = model.classify_nodes(g, labels, lambdas=args.classify or None, folds=F, fold=fold.to(device))
            g.ndata['h'] = features
            with torch.no_grad():
                z = model.encode(g)
            g.ndata['h'] = features
            z = z[0] if isinstance(z, tuple) else z
            zt = z.index_select(0, test.to(device)).contiguous()
            pred, proba = ops.logreg_predict(zt, res.coef, res.intercept, res.pivot, proba=True)
            cm = metrics.classification_metrics(pred, labels[test.to(device)], proba, n_classes=res.coef.shape[0])
            print(f"LogReg ({F}-fold CV, lambda = {res.lam:g}) test accuracy: {cm['accuracy']:.4f} | "
                  f"macro-F1: {cm['macro_f1']:.4f} | log-loss: {cm['log_loss']:.4f}")
            main.last_classify = {"result": res, "metrics": cm, "test": test, "pred": pred}
            if args.classify_out is not None:
                np.savez(args.classify_out, coef=res.coef.cpu().numpy(), intercept=res.intercept.cpu().numpy(), lam=res.lam,
                         lambdas=res.lambdas.cpu().numpy(), cv_logloss=res.cv_logloss.cpu().numpy(),
                         cv_accuracy=res.cv_accuracy.cpu().numpy(), test_index=test.numpy(), test_pred=pred.cpu().numpy())
    if args.map_out is not None:
        import numpy as np
        P = 20.0 if args.map_perplexity is None else args.map_perplexity
        T = 1000 if args.map_iters is None else args.map_iters
        g.ndata['h'] = features
        res = model.map_nodes(g, perplexity=P, n_iter=T, seed=args.map_seed or 0,
                              init="pca" if args.map_init == "pca" else None)
        g.ndata['h'] = features
        k10 = min(10, n_nodes - 1)
        keep = metrics.neighbourhood_preservation(model.nearest_nodes(g, k10).index, ops.knn(res.embedding, k=k10).index)
        g.ndata['h'] = features
        print(f"t-SNE (perplexity {P:g}, {res.n_iter} iterations) KL: {res.kl_divergence:.4f} | "
              f"10-NN preservation: {keep:.4f}")
        labels = np.full(n_nodes, -1, np.int64) if data.labels is None else np.asarray(data.labels, np.int64)
        np.savez(args.map_out, embedding=res.embedding.cpu().numpy(), labels=labels, kl_divergence=res.kl_divergence,
                 kl_curve=np.asarray(res.kl_curve, np.float64).reshape(-1, 2))
        main.last_map = {"result": res, "preservation": keep}
    if args.pca is not None:
        import numpy as np
        g.ndata['h'] = features
        res = model.pca_nodes(g, args.pca)
        g.ndata['h'] = features
        ratio = res.explained_variance_ratio.cpu().numpy()
        print(f"PCA ({args.pca} of {res.components.shape[1]} components) explained variance: "
              f"{' '.join(f'{v:.4f}' for v in ratio)} (cumulative {float(ratio.sum()):.4f})")
        if args.pca_out is not None:
            with torch.no_grad():
                z = model.encode(g)
            g.ndata['h'] = features
            z = z[0] if isinstance(z, tuple) else z
            np.savez(args.pca_out, components=res.components.cpu().numpy(), mean=res.mean.cpu().numpy(),
                     explained_variance=res.explained_variance.cpu().numpy(), explained_variance_ratio=ratio,
                     scores=res.transform(z).cpu().numpy())
        main.last_pca = res
    if args.spectral is not None:
        import numpy as np
        K = args.spectral
        sc = ops.spectral_embedding(g, K, self_loops=args.spectral_self_loops, scaling=args.spectral_scaling or "none",
                                    seed=args.spectral_seed or 0)
        main.last_spectral = {"result": sc}
        for name, pairs in held_out.items():
            scores = metrics.evaluate(sc.embedding, pairs)
            print(f"spectral ({K}) {name} ROC-AUC: {scores['auc']:.4f} | AP: {scores['ap']:.4f}")
            main.last_spectral[name] = scores
        if args.cluster is not None:
            res = ops.kmeans(sc.embedding, args.cluster, seed=args.cluster_seed or 0)
            print(f"spectral k-means K = {args.cluster}: inertia {res.inertia:.6g} | iterations: {res.n_iter}"
                  f"{'' if res.converged else ' (not converged)'} | sizes: {res.counts.tolist()}")
            main.last_spectral["cluster"] = {"result": res}
            if data.labels is not None:
                cm = metrics.clustering_metrics(res.labels.cpu().numpy(), data.labels)
                print(f"spectral NMI: {cm['nmi']:.4f} | ARI: {cm['ari']:.4f} | ACC: {cm['acc']:.4f}")
                main.last_spectral["cluster"].update(cm)
        if args.classify is not None and main.last_classify is not None:
            # the split and the folds of the model's own head, so the two lines compare like with like
            test = main.last_classify["test"]
            labels = torch.as_tensor(data.labels, dtype=torch.int64, device=device)
            F = args.classify_folds or 5
            res = ops.logreg(sc.embedding, labels, lambdas=args.classify or None, folds=F, fold=fold.to(device))
            zt = sc.embedding.index_select(0, test.to(device)).contiguous()
            pred, proba = ops.logreg_predict(zt, res.coef, res.intercept, res.pivot, proba=True)
            cm = metrics.classification_metrics(pred, labels[test.to(device)], proba, n_classes=res.coef.shape[0])
            print(f"spectral LogReg ({F}-fold CV, lambda = {res.lam:g}) test accuracy: {cm['accuracy']:.4f} | "
                  f"macro-F1: {cm['macro_f1']:.4f} | log-loss: {cm['log_loss']:.4f}")
            main.last_spectral["classify"] = {"result": res, "metrics": cm, "pred": pred}
        if args.spectral_out is not None:
            np.savez(args.spectral_out, embedding=sc.embedding.cpu().numpy(), vectors=sc.vectors.cpu().numpy(),
                     values=sc.values.cpu().numpy(), residuals=sc.residuals.cpu().numpy())
    if args.deepwalk is not None:
        import numpy as np
        D = args.deepwalk
        dw = ops.deepwalk(g, D, walks_per_node=args.deepwalk_walks or 10, walk_length=args.deepwalk_length or 40,
                          window=args.deepwalk_window or 5, epochs=args.deepwalk_epochs or 3, seed=args.deepwalk_seed or 0)
        main.last_deepwalk = {"result": dw}
        for name, pairs in held_out.items():
            scores = metrics.evaluate(dw.embedding, pairs)
            print(f"deepwalk ({D}) {name} ROC-AUC: {scores['auc']:.4f} | AP: {scores['ap']:.4f}")
            main.last_deepwalk[name] = scores
        if args.cluster is not None:
            res = ops.kmeans(dw.embedding, args.cluster, seed=args.cluster_seed or 0)
            print(f"deepwalk k-means K = {args.cluster}: inertia {res.inertia:.6g} | iterations: {res.n_iter}"
                  f"{'' if res.converged else ' (not converged)'} | sizes: {res.counts.tolist()}")
            main.last_deepwalk["cluster"] = {"result": res}
            if data.labels is not None:
                cm = metrics.clustering_metrics(res.labels.cpu().numpy(), data.labels)
                print(f"deepwalk NMI: {cm['nmi']:.4f} | ARI: {cm['ari']:.4f} | ACC: {cm['acc']:.4f}")
                main.last_deepwalk["cluster"].update(cm)
        if args.classify is not None and main.last_classify is not None:
            # the split and the folds of the model's own head, so the two lines compare like with like
            test = main.last_classify["test"]
            labels = torch.as_tensor(data.labels, dtype=torch.int64, device=device)
            F = args.classify_folds or 5
            res = ops.logreg(dw.embedding, labels, lambdas=args.classify or None, folds=F, fold=fold.to(device))
            zt = dw.embedding.index_select(0, test.to(device)).contiguous()
            pred, proba = ops.logreg_predict(zt, res.coef, res.intercept, res.pivot, proba=True)
            cm = metrics.classification_metrics(pred, labels[test.to(device)], proba, n_classes=res.coef.shape[0])
            print(f"deepwalk LogReg ({F}-fold CV, lambda = {res.lam:g}) test accuracy: {cm['accuracy']:.4f} | "
                  f"macro-F1: {cm['macro_f1']:.4f} | log-loss: {cm['log_loss']:.4f}")
            main.last_deepwalk["classify"] = {"result": res, "metrics": cm, "pred": pred}
        if args.deepwalk_out is not None:
            np.savez(args.deepwalk_out, embedding=dw.embedding.cpu().numpy(), context=dw.context.cpu().numpy(),
                     walks=dw.walks.cpu().numpy(), counts=dw.counts.cpu().numpy())
    if args.heuristics is not None:
        import numpy as np
        kinds = list(dict.fromkeys(args.heuristics)) or list(HEURISTIC_KINDS)
        weights = ops.neighbour_weights(g)                 # the training graph: held-out edges are not in it
        main.last_heuristics = {}
        tables = {}
        for name, split in held_out.items():
            ns = {part: ops.neighbour_scores(g, torch.as_tensor(split[part], device=device), weights=weights)
                  for part in ("pos", "neg")}
            for part in ("pos", "neg"):
                tables[f"{name}_{part}_pairs"] = np.asarray(split[part], np.int64)
                for field in ["common", "deg_i", "deg_j"] + kinds:
                    tables[f"{name}_{part}_{field}"] = getattr(ns[part], field).cpu().numpy()
            for kind in kinds:
                scores = metrics.evaluate_scores(getattr(ns["pos"], kind), getattr(ns["neg"], kind))
                print(f"{kind} {name} ROC-AUC: {scores['auc']:.4f} | AP: {scores['ap']:.4f}")
                main.last_heuristics[(kind, name)] = scores
        if args.topk is not None:
            for kind in kinds:
                if kind == "pa":                           # not a local score: no top-k
                    continue
                top = ops.neighbour_topk(g, args.topk, kind, weights=weights)
                recall = metrics.recall_at_k(top.index, held_out["test"]["pos"])
                print(f"{kind} test recall@{args.topk}: {recall:.4f}")
                main.last_heuristics[(kind, "recall")] = recall
        if args.heuristics_out is not None:
            np.savez(args.heuristics_out, **tables)
    return [float(l) for l in losses]


if __name__ == '__main__':
    main()
