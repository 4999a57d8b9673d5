"""Host-side mirror of the reference model file gae_dgl/gae.py: same class
names, constructor arguments, attribute names and state-dict keys
(``layers.{i}.apply_mod.linear.{weight,bias}``), same side effects on
``g.ndata['h']`` -- with every arithmetic op executed by the HIP kernels of
libgae_hip.so (SpMM, fp32-MFMA Linear+activation, inner-product decoder).

Extensions over the reference are keyword-only: ``norm="none"|"both"``
(gae.py applies no normalisation although train_transductive.py:55-58
computes one), an injectable dropout mask/seed for reproducible tests, and
the evaluation ORDER of a layer that narrows wide features (layer 1: 500 /
1433 / 3703 -> 32): ``transform_first=None`` (default, "auto") evaluates
such a layer as ``act(A (H W^T) + b)`` -- the value of the reference's
``act((A H) W^T + b)`` up to fp32 rounding (2e-7 of the scale measured; the
parity suite holds it to the same 1e-5 as everything else) -- because the
aggregation then runs at the OUTPUT width and the 40 MB aggregate ``A H`` is
neither written nor re-read (gae_xw_fwd / gae_spmm_csr_epilogue /
gae_xw_wgrad); ``transform_first=False`` keeps the reference's order
everywhere, ``True`` asks for the reorder on every narrowing layer (it takes
effect wherever the one-pass kernels apply, like "auto").  ``cache_aggregate``
(opt-in) keeps ``A H`` of a parameter-independent input across steps."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import function as fn
from . import ops
from .sparse import SparseFeatures
from ._lib import ACT_IDENTITY, ACT_RELU


# GCN layers with <= 64 input and <= 32 output features run as ONE launch (gae_gcn_layer_fused: aggregation + Linear +
# bias + activation, backward of the identity-activation layer likewise) when the graph carries a packed neighbour
# table; False restores the two launches per layer (update_all, apply_nodes) everywhere.  Same values up to fp32
# rounding of the 32 -> 16 product.
FUSE_NARROW_LAYERS = True
# Layers that narrow WIDE features (f_in >= 193, f_out <= 32) built with transform_first=None run as
# act(A (H W^T) + b) through the one-pass kernels; False makes "auto" mean the reference's order (experiments)
TRANSFORM_FIRST_AUTO = True


def identity(x):
    return x


def _act_code(activation):
    """fused-epilogue code of an activation callable, or None (apply it after)"""
    if activation is None or activation is identity:
        return ACT_IDENTITY
    if activation is F.relu or activation is torch.relu:
        return ACT_RELU
    if getattr(activation, "__name__", "") == "<lambda>":
        # the reference spells identity as ``lambda x: x`` (gae.py:43,45,47)
        code = getattr(activation, "__code__", None)
        if code is not None and code.co_argcount == 1 and code.co_code == (lambda x: x).__code__.co_code:
            return ACT_IDENTITY
    return None


class NodeApplyModule(nn.Module):
    """gae.py:7-16 -- Linear (+bias) then activation, as one fused HIP kernel."""

    def __init__(self, in_feats, out_feats, activation):
        super().__init__()
        self.linear = nn.Linear(in_feats, out_feats)  # default init, weight [out, in] (gae.py:10)
        self.activation = activation

    def forward(self, node):
        feats = node.data['h']
        if feats.dtype != torch.float32:  # bf16-stored features: aggregation ran in bf16 storage / fp32 accumulate
            feats = ops.float_rows(feats) if feats.is_cuda and feats.dim() == 2 else feats.float()
        fused = _act_code(self.activation)
        out = ops.linear(feats, self.linear.weight, self.linear.bias, ACT_IDENTITY if fused is None else fused)
        return {'h': out if fused is not None else self.activation(out)}


# the message / reduce pair the reference hands to update_all (gae.py:18-19): copy the source feature, sum it
gcn_msg, gcn_reduce = fn.copy_src(src='h', out='m'), fn.sum(msg='m', out='h')


class GCN(nn.Module):
    """gae.py:21-31 -- aggregate over in-edges (HIP SpMM) -> NodeApplyModule.

    ``transform_first`` (opt-in, layers that narrow the features only): ``act(A (H W^T) + b)``.  Mathematically the
    reference's ``act((A H) W^T + b)``; the rounding differs (measured 2e-7 relative), the aggregation moves
    F_out instead of F_in floats per edge and nothing of width F_in is written.
    ``cache_aggregate`` (opt-in): reuse ``A H`` while the same parameter-free input tensor comes back unchanged."""

    def __init__(self, in_feats, out_feats, activation, norm=None, *, transform_first=None, cache_aggregate=False):
        super().__init__()
        self.norm = norm
        self.apply_mod = NodeApplyModule(in_feats, out_feats, activation)
        # True: reorder whenever the layer narrows; None ("auto"): reorder where the one-pass kernels apply (wide
        # input, <= 32 outputs, graph with a packed neighbour table); False: the reference's order
        self.transform_first = bool(transform_first) and in_feats > out_feats
        self.transform_auto = transform_first is None and in_feats > out_feats and not cache_aggregate
        self.cache_aggregate = bool(cache_aggregate)
        self._agg_key = self._agg = None

    def _one_pass(self, g, feature):
        """the layer through ops.GCNTransformFirstFunction, or None when shapes / graph do not allow it"""
        code = _act_code(self.apply_mod.activation)
        if code is None or not isinstance(feature, torch.Tensor) or not feature.is_cuda:
            return None
        g._follow(feature)
        mode = g.norm_mode if self.norm is None else self.norm
        if mode not in ("none", "both"):
            return None
        lin = self.apply_mod.linear
        return ops.gcn_layer_transform_first(g, feature, lin.weight, lin.bias, code, use_norm=(mode == "both"))

    def _forward_sparse_input(self, g, sf):
        """``feature`` is a sparse.SparseFeatures (compressed input): the layer from its non-zeros, or from its dense
        form when the one-pass route does not apply"""
        code = _act_code(self.apply_mod.activation)
        if sf.device != g.device and sf.device.type == "cuda":
            g.to(sf.device)
        mode = g.norm_mode if self.norm is None else self.norm
        lin = self.apply_mod.linear
        if code is not None and mode in ("none", "both"):
            g.ndata['h'] = sf                    # same traffic on g.ndata['h'] as the dense path (gae.py:27,30)
            out = ops.gcn_layer_sparse_input(g, sf, lin.weight, lin.bias, code, use_norm=(mode == "both"))
            if out is not None:
                g.ndata.pop('h')
                return out
        return self.forward(g, sf.to_dense(cache=True))      # (constant features: densified once, then reused)

    def forward(self, g, feature):
        if isinstance(feature, SparseFeatures):
            return self._forward_sparse_input(g, feature)
        # same traffic on g.ndata['h'] as the reference: set (gae.py:27), reduced in place (:28), transformed in
        # place (:29), removed (:30)
        g.ndata['h'] = feature
        code = _act_code(self.apply_mod.activation)
        if self.transform_first or (self.transform_auto and TRANSFORM_FIRST_AUTO):
            # (where the one-pass kernels do not apply -- narrow inputs, graphs with heavy rows -- the layer keeps
            #  the reference's order)
            out = self._one_pass(g, feature)
            if out is not None:
                g.ndata.pop('h')
                return out
        if FUSE_NARROW_LAYERS and code is not None and not self.cache_aggregate and isinstance(feature, torch.Tensor) \
                and feature.is_cuda:
            g._follow(feature)
            mode = g.norm_mode if self.norm is None else self.norm
            lin = self.apply_mod.linear
            out = ops.gcn_layer(g, feature, lin.weight, lin.bias, code, use_norm=(mode == "both")) \
                if mode in ("none", "both") else None
            if out is not None:
                g.ndata.pop('h')
                return out
        if self.cache_aggregate and not feature.requires_grad:
            key = (id(g), g.number_of_edges(), feature.data_ptr(), feature._version, tuple(feature.shape), self.norm)
            if self._agg_key != key:
                g.update_all(gcn_msg, gcn_reduce, norm=self.norm)
                self._agg_key, self._agg = key, g.ndata['h']
            g.ndata['h'] = self._agg
        else:
            g.update_all(gcn_msg, gcn_reduce, norm=self.norm)
        g.apply_nodes(func=self.apply_mod)
        return g.ndata.pop('h')


_UNSET = object()


def reconstruct_threshold(prob=_UNSET, threshold=None):
    """the logit threshold of ``reconstruct(prob=..., threshold=...)``: exactly one of the two may be given (neither:
    prob = 0.5); ``prob`` in (0, 1) becomes log(p / (1 - p)), computed in fp64 and rounded to fp32 (0.5 -> exactly 0.0)"""
    if threshold is not None:
        if prob is not _UNSET and prob is not None:
            raise ValueError("reconstruct: give prob or threshold, not both")
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("reconstruct: threshold is NaN")
        return threshold
    return ops.threshold_of_prob(0.5 if prob is _UNSET or prob is None else prob)


def reconstruct_embedding(z, g, threshold, scope, exclude_self, exclude_edges, max_pairs):
    """ops.decoder_threshold on a given embedding: what GAE.reconstruct does with Z and VGAE.reconstruct with mu"""
    z = z.detach()
    if z.dtype != torch.float32:
        z = z.float()
    return ops.decoder_threshold(z, threshold, g, scope=scope, exclude_self=exclude_self, exclude_edges=exclude_edges,
                                 max_pairs=max_pairs)


def _empty_scores(B, dev):
    f64 = lambda: torch.empty(B, dtype=torch.float64, device=dev)       # noqa: E731
    i64 = lambda: torch.empty(B, dtype=torch.int64, device=dev)         # noqa: E731
    return ops.GraphScores(torch.empty(B, dtype=torch.float32, device=dev), f64(), f64(), i64(), i64(), i64(), i64())


def _put_scores(full, where, part):
    for dst, src in zip(full, part):
        dst[where] = src


def score_embedding(z, g, exclude_self=True, members=None):
    """``ops.GraphScores`` of the member graphs of the batched graph ``g`` (``members``: their positions, default all)
    for a GIVEN node embedding ``z`` [N, d]: members of at most 64 nodes through the no-layer mode of ops.score_graphs
    (d <= 64), the others one by one through metrics.graph_scores_dense.  What GAE.score_graphs does with the Z of its
    chunked route and VGAE.score_graphs with mu."""
    import numpy as np
    from . import metrics
    z = z.detach()
    if z.dtype != torch.float32:
        z = z.float()
    g._follow(z)
    dev = z.device
    counts = g.batch_num_nodes if g.batch_num_nodes is not None else [g.number_of_nodes()]
    sizes = np.asarray(counts, dtype=np.int64)
    members = np.arange(len(sizes), dtype=np.int64) if members is None else np.asarray(members, dtype=np.int64)
    B = len(members)
    gp, (indptr, indices) = g.graph_ptr(), g.csr()
    small = sizes[members] <= ops.EMBED_MAX_NODES
    if not ops.score_graphs_usable(z.shape[1], [], 0):
        small[:] = False
    out = None
    if small.any():
        whole = bool(small.all()) and B == len(sizes) and bool((members == np.arange(B)).all())
        gids = None if whole else torch.from_numpy(np.ascontiguousarray(members[small])).to(dev)
        out = ops.score_graphs(gp, indptr, indices, z, graph_ids=gids, max_graph_nodes=int(sizes[members][small].max()),
                               exclude_self=exclude_self)
        if small.all():
            return out
    full = _empty_scores(B, dev)
    if out is not None:
        _put_scores(full, torch.from_numpy(np.nonzero(small)[0]).to(dev), out)
    gp_host = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=gp_host[1:])
    for k in np.nonzero(~small)[0]:
        r0, r1 = int(gp_host[members[k]]), int(gp_host[members[k] + 1])
        e0, e1 = int(indptr[r0]), int(indptr[r1])
        row = metrics.graph_scores_dense(z[r0:r1], (indptr[r0:r1 + 1].long() - e0, indices[e0:e1].long() - r0), exclude_self)
        for name, t in zip(full._fields, full):
            t[k] = row[name]
    return full


class GAE(nn.Module):
    """gae.py:33-61.  ReLU on layers 0..L-2, identity on the last layer; a
    single hidden dim gives one identity layer (gae.py:36-45)."""

    def __init__(self, in_dim, hidden_dims, *, norm=None, transform_first=None, cache_first_aggregate=False):
        super().__init__()
        widths = [in_dim] + list(hidden_dims)
        last = len(widths) - 2
        self.layers = nn.ModuleList(
            GCN(widths[k], widths[k + 1], identity if k == last else F.relu, norm, transform_first=transform_first,
                cache_aggregate=cache_first_aggregate and k == 0) for k in range(last + 1))
        self.decoder = InnerProductDecoder(activation=identity)

    def _embed(self, g, write_back):
        z = g.ndata['h']
        for layer in self.layers:
            z = layer(g, z)
        if write_back:
            g.ndata['h'] = z     # forward() leaves the embedding on the graph (gae.py:53); encode() does not
        return z

    def forward(self, g):
        return self.decoder(self._embed(g, write_back=True))

    def encode(self, g):
        return self._embed(g, write_back=False)

    def predict_links(self, g, k, *, scope="batch", exclude_self=True, exclude_edges=True):
        """(score [n, k], index [n, k]): the k most likely new neighbours of every node -- the largest logits
        z_i . z_j of the decoder (gae.py:69-72, no dropout) among the pairs that are not edges of ``g`` -- from one
        fused HIP launch (ops.decoder_topk) that never forms the N x N matrix.  ``sigmoid(score)`` is the probability.
        ``scope="graph"``: only inside each member graph of a batched ``g``.  Rows with fewer than k candidates pad
        with index -1 / score -inf.  Runs encode(g) under no_grad; g.ndata is left as encode() leaves it."""
        with torch.no_grad():
            z = self.encode(g)
        return ops.decoder_topk(z, k, g, scope=scope, exclude_self=exclude_self, exclude_edges=exclude_edges)

    def rank_links(self, g, pairs, *, filter_graph=None, scope="batch", exclude_self=True, exclude_edges=True):
        """RankResult(score, greater, equal, candidates), one entry per query pair (i, j) of ``pairs`` [2, m]: the logit
        z_i . z_j and how many candidates c of i (the candidate rule of predict_links, j itself left out) score above /
        exactly at it -- the filtered rank of j among ALL candidates of i, from one fused HIP launch
        (ops.decoder_rank) that never forms an m x N matrix.  ``filter_graph`` (default ``g``) supplies the edges that
        are left out: pass the full graph to filter the held-out edges too; the target itself is always ranked.
        ``metrics.rank_metrics`` gives MRR, Hits@K, mean rank and the all-negatives AUC.  Runs encode(g) under
        no_grad; g.ndata is left as encode() leaves it."""
        with torch.no_grad():
            z = self.encode(g)
        return ops.decoder_rank(z, pairs, g, filter_graph=filter_graph, scope=scope, exclude_self=exclude_self,
                                exclude_edges=exclude_edges)

    def reconstruct(self, g, *, prob=_UNSET, threshold=None, scope="batch", exclude_self=True, exclude_edges=False,
                    max_pairs=2 ** 27):
        """``ops.DecodedLinks(indptr, index, score)``: the reconstructed graph A_hat = 1[sigmoid(z_i . z_j) >= prob]
        of the decoder (gae.py:69-72, no dropout) as a CSR -- row i lists, columns ascending, the nodes j whose logit
        z_i . z_j reaches the threshold, with the logits -- from the fused HIP launches of ops.decoder_threshold that
        never form the N x N matrix.  Give ``prob`` in (0, 1) (default 0.5) or the logit ``threshold`` itself, not both.
        ``scope="graph"``: every member of a batched ``g`` is decoded inside its own window.  ``exclude_edges`` lists
        only pairs that are not edges of ``g`` (new links); ``max_pairs`` bounds the output (GaeHipError beyond it).
        ``metrics.reconstruction_metrics`` compares the result with the graph.  Runs encode(g) under no_grad;
        ``g.ndata['h']`` is restored on exit."""
        t = reconstruct_threshold(prob, threshold)
        feat = g.ndata['h']
        with torch.no_grad():
            try:
                z = self.encode(g)
            finally:
                g.ndata['h'] = feat
        return reconstruct_embedding(z, g, t, scope, exclude_self, exclude_edges, max_pairs)

    def cluster_nodes(self, g, k, **kw):
        """``ops.KMeansResult``: node clustering, the second downstream task of a graph auto-encoder -- k-means with
        ``k`` clusters on the embedding encode(g), on the device (ops.kmeans; its keyword arguments pass through:
        init, n_init, max_iter, tol, seed, check_every).  ``metrics.clustering_metrics`` scores the labels against
        classes.  Runs encode(g) under no_grad; ``g.ndata['h']`` is restored on exit."""
        feat = g.ndata['h']
        with torch.no_grad():
            try:
                z = self.encode(g)
            finally:
                g.ndata['h'] = feat
        return ops.kmeans(z, k, **kw)

    def nearest_nodes(self, g, k, *, metric="l2"):
        """``ops.KNNResult(index, value)``: the ``k`` nearest nodes of every node in the embedding encode(g), the node
        itself left out -- exact, on the device (ops.knn), without the N x N distance matrix.  ``metric``: "l2"
        (squared distance, ascending), "dot" or "cosine" (descending).  ``metrics.knn_predict`` turns the lists and
        class labels into the leave-one-out kNN accuracy of the embedding.  Runs encode(g) under no_grad;
        ``g.ndata['h']`` is restored on exit."""
        feat = g.ndata['h']
        with torch.no_grad():
            try:
                z = self.encode(g)
            finally:
                g.ndata['h'] = feat
        return ops.knn(z, k=k, metric=metric)

    def map_nodes(self, g, **kw):
        """``ops.TSNEResult``: the 2-D map of the embedding encode(g) -- the Cora figure of the GAE / VGAE papers -- by
        exact t-SNE on the device (ops.tsne; its keyword arguments pass through: perplexity, n_iter, learning_rate,
        early_exaggeration, exaggeration_iters, seed, init, neighbours, min_grad_norm, check_every).
        ``metrics.neighbourhood_preservation`` scores the map against the embedding.  Runs encode(g) under no_grad;
        ``g.ndata['h']`` is restored on exit."""
        feat = g.ndata['h']
        with torch.no_grad():
            try:
                z = self.encode(g)
            finally:
                g.ndata['h'] = feat
        return ops.tsne(z, **kw)

    def map_graphs(self, data, **kw):
        """``ops.TSNEResult``: the 2-D map of the molecule features of ``embed_graphs`` by exact t-SNE on the device
        (``ops.tsne``; its keyword arguments pass through).  ``fused`` and ``batch_size`` go to the embedding.  Rows are
        in the order ``embed_graphs(data)`` returns them.  Runs under no_grad."""
        if "grad" in kw:
            raise ValueError("map_graphs runs under no_grad: the map carries no gradient into the encoder")
        embed_kw = {k: kw.pop(k) for k in ("fused", "batch_size") if k in kw}
        with torch.no_grad():
            return ops.tsne(self.embed_graphs(data, **embed_kw), **kw)

    def pca_nodes(self, g, k=None, **kw):
        """``ops.PCAResult``: the ``k`` leading principal components of the embedding encode(g) (default: all) -- the
        explained-variance spectrum, a linear projection (``result.transform(z)``), whitening -- on the device
        (ops.pca; its keyword arguments pass through: rows, whiten, pivot).  Runs encode(g) under no_grad;
        ``g.ndata['h']`` is restored on exit."""
        feat = g.ndata['h']
        with torch.no_grad():
            try:
                z = self.encode(g)
            finally:
                g.ndata['h'] = feat
        return ops.pca(z, k, **kw)

    def pca_graphs(self, data, k=None, **kw):
        """``ops.PCAResult``: the ``k`` leading principal components of the molecule features of ``embed_graphs`` on the
        device (``ops.pca``; its keyword arguments pass through).  ``fused`` and ``batch_size`` go to the embedding.  Rows
        are in the order ``embed_graphs(data)`` returns them.  Runs under no_grad."""
        if "grad" in kw:
            raise ValueError("pca_graphs runs under no_grad: the decomposition carries no gradient into the encoder")
        embed_kw = {key: kw.pop(key) for key in ("fused", "batch_size") if key in kw}
        with torch.no_grad():
            return ops.pca(self.embed_graphs(data, **embed_kw), k, **kw)

    def classify_nodes(self, g, labels, **kw):
        """``ops.LogRegResult``: the standard protocol for an unsupervised node embedding -- freeze encode(g), fit a
        multinomial logistic regression on the labelled nodes (``labels``: an int tensor [n], -1 = unlabelled), choose
        the penalty by k-fold CV, on the device (ops.logreg; its keyword arguments pass through: lambdas, folds, fold,
        seed, n_classes, max_iter, tol, check_every, model_batch; ``fold = -1`` keeps a test set out).
        ``metrics.classification_metrics`` scores ``result.predict(z)`` on the nodes kept out.  Runs encode(g) under
        no_grad; ``g.ndata['h']`` is restored on exit."""
        feat = g.ndata['h']
        with torch.no_grad():
            try:
                z = self.encode(g)
            finally:
                g.ndata['h'] = feat
        return ops.logreg(z, labels, **kw)

    def nearest_graphs(self, data, k, *, queries=None, metric="l2", **embed_kw):
        """``ops.KNNResult(index, value)``: similarity search over the molecule features of ``embed_graphs`` (its
        keyword arguments pass through: fused, batch_size).  ``queries=None``: the kNN graph of ``data`` -- for every
        graph its ``k`` nearest other graphs.  Otherwise the graphs of ``queries`` (a set, a ``subset()`` view or a
        batched graph) are searched against ``data``; a graph that is in both is its own nearest neighbour.  The
        indices are rows of ``data`` in the order ``embed_graphs(data)`` returns them.  Runs under no_grad."""
        if "grad" in embed_kw:
            raise ValueError("nearest_graphs runs under no_grad: the neighbour lists carry no gradient")
        with torch.no_grad():
            X = self.embed_graphs(data, **embed_kw)
            if queries is None:
                return ops.knn(X, k=k, metric=metric)
            return ops.knn(self.embed_graphs(queries, **embed_kw), X, k=k, metric=metric)

    def ridge_graphs(self, data, y, **kw):
        """``ops.RidgeResult``: ridge regression of the per-molecule targets ``y`` ([G] or [G, t]) on the molecule
        features of ``embed_graphs`` -- the reference's "GAE + Ridge" head, lambda chosen by k-fold CV on the device
        (``ops.ridge``; its keyword arguments pass through: lambdas, folds, fold, seed, fit_intercept, pivot).  ``fused``
        and ``batch_size`` go to the embedding.  Rows are in the order ``embed_graphs(data)`` returns them.  Runs under
        no_grad."""
        if "grad" in kw:
            raise ValueError("ridge_graphs runs under no_grad: the closed-form fit carries no gradient")
        embed_kw = {k: kw.pop(k) for k in ("fused", "batch_size") if k in kw}
        with torch.no_grad():
            return ops.ridge(self.embed_graphs(data, **embed_kw), y, **kw)

    def logreg_graphs(self, data, y, **kw):
        """``ops.LogRegResult``: multinomial logistic regression of the per-molecule classes ``y`` (an int tensor [G], -1 =
        unlabelled) on the molecule features of ``embed_graphs`` -- the head of a classification property, lambda chosen
        by k-fold CV on the device (``ops.logreg``; its keyword arguments pass through: lambdas, folds, fold, seed,
        n_classes, max_iter, tol, check_every, model_batch).  ``fused`` and ``batch_size`` go to the embedding.  Rows are
        in the order ``embed_graphs(data)`` returns them.  Runs under no_grad."""
        if "grad" in kw:
            raise ValueError("logreg_graphs runs under no_grad: the fitted head carries no gradient into the encoder")
        embed_kw = {k: kw.pop(k) for k in ("fused", "batch_size") if k in kw}
        with torch.no_grad():
            return ops.logreg(self.embed_graphs(data, **embed_kw), y, **kw)

    def forest_graphs(self, data, y, **kw):
        """``ops.ForestResult``: a random forest regression of the per-molecule targets ``y`` ([G] or [G, t]) on the
        molecule features of ``embed_graphs`` -- the reference's "GAE + Random Forest" head, grown on the device with its
        out-of-bag scores (``ops.forest``; its keyword arguments pass through: n_trees, max_depth, max_features,
        min_samples_leaf, max_bins, bootstrap, max_samples, rows, seed).  ``fused`` and ``batch_size`` go to the embedding.
        Rows are in the order ``embed_graphs(data)`` returns them.  Runs under no_grad."""
        if "grad" in kw:
            raise ValueError("forest_graphs runs under no_grad: a forest carries no gradient")
        embed_kw = {k: kw.pop(k) for k in ("fused", "batch_size") if k in kw}
        with torch.no_grad():
            return ops.forest(self.embed_graphs(data, **embed_kw), y, **kw)

    def boost_graphs(self, data, y, objective="squared", n_rounds=100, **kw):
        """``ops.BoostResult``: gradient-boosted histogram trees on the molecule features of ``embed_graphs`` for the
        per-molecule targets ``y`` (fp32 [G] with ``objective="squared"``; an int tensor [G] in {0, 1}, -1 = unlabelled,
        with ``"logistic"``), the learning rate, lambda and the number of rounds chosen by k-fold CV on the device
        (``ops.boost``; its keyword arguments pass through: max_depth, learning_rates, lambdas, min_child_weight,
        min_samples_leaf, min_gain, max_features, max_bins, folds, fold, rows, seed, check_every, oof).  ``fused`` and
        ``batch_size`` go to the embedding.  Rows are in the order ``embed_graphs(data)`` returns them.  Runs under no_grad."""
        if "grad" in kw:
            raise ValueError("boost_graphs runs under no_grad: boosted trees carry no gradient")
        embed_kw = {k: kw.pop(k) for k in ("fused", "batch_size") if k in kw}
        with torch.no_grad():
            return ops.boost(self.embed_graphs(data, **embed_kw), y, objective, n_rounds, **kw)

    def mlp_graphs(self, data, y, **kw):
        """``ops.MLPResult``: an MLP regression of the per-molecule targets ``y`` ([G] or [G, t]) on the molecule features
        of ``embed_graphs`` -- the reference's "GAE + MLP" head, every fold model of every (lr, alpha) pair trained side
        by side on the device (``ops.mlp``; its arguments pass through: hidden, lrs, alphas, epochs, batch_size, folds,
        fold, ensemble, seed, solver, momentum, shuffle, standardize).  ``fused`` and ``embed_batch_size`` go to the
        embedding (``batch_size`` is the head's mini-batch).  Rows are in the order ``embed_graphs(data)`` returns them.
        Runs under no_grad."""
        if "grad" in kw:
            raise ValueError("mlp_graphs runs under no_grad: the trained head carries no gradient into the encoder")
        embed_kw = {}
        if "fused" in kw:
            embed_kw["fused"] = kw.pop("fused")
        if "embed_batch_size" in kw:
            embed_kw["batch_size"] = kw.pop("embed_batch_size")
        with torch.no_grad():
            return ops.mlp(self.embed_graphs(data, **embed_kw), y, **kw)

    def embed_graphs(self, data, *, fused="auto", batch_size=4096, grad=False):
        """fp32 [n_graphs, 3 d]: the molecule feature of the reference's chemistry table (README.md:54: mean | sum |
        max of the hidden vectors, 48 numbers for ``--hidden_dims 32 16``) of every graph of ``data`` -- a
        ``DeviceGraphDataset`` or a ``subset()`` view (rows in the order of ``data.ids``), or a batched graph with
        ``graph_ptr()`` and ``ndata['h']`` (rows in member order).  Parameters and ``g.ndata`` are left as they were.
        The norm follows the model as in encode(): ``GAE(norm=...)`` if given, else the graph's ``norm_mode`` (the
        batches of a dataset carry "none").
        ``fused=True``: one launch for the whole set (ops.embed_graphs: encoder and readout per molecule, nothing of
        width N written); raises when the model or a graph lies outside the kernel's shapes (1..4 layers, widths <= 64,
        graphs <= 64 nodes).  ``fused=False``: ``batch`` -> ``encode`` -> ``readout_nodes`` in chunks of ``batch_size``
        graphs.  ``"auto"``: the kernel for every graph it takes, the chunked route for the rest.
        ``grad=False`` (default) runs under no_grad.  ``grad=True`` runs with autograd, for fine-tuning the encoder
        through the features: the same forward values bit for bit, and a result whose backward reaches the encoder's
        parameters -- through the kernel pair gae_embed_graphs / gae_embed_graphs_bwd (K19 / K21) where ``fused`` says
        so (``True``: the pair or an error; ``"auto"``: the pair for every graph BOTH kernels take), through the
        chunked route and the readout's own backward elsewhere; the rows are scattered into place with differentiable
        indexing."""
        if fused not in ("auto", True, False):
            raise ValueError(f"fused: 'auto', True or False, not {fused!r}")
        if isinstance(batch_size, bool) or int(batch_size) != batch_size or batch_size < 1:
            raise ValueError(f"batch_size: a positive number of graphs, not {batch_size!r}")
        if grad not in (True, False):
            raise ValueError(f"grad: True or False, not {grad!r}")
        with torch.set_grad_enabled(bool(grad)):
            return self._embed_graphs(data, fused, int(batch_size), grad=bool(grad))

    def _graph_set(self, data, who):
        """what embed_graphs / score_graphs read of ``data`` (a resident set or a batched graph) and what the model
        allows: (is_set, ids, sizes, identity_ids, feat, mode, codes, why) -- ``why`` names what keeps the model out of
        the fused kernels (None: taken)"""
        import numpy as np
        is_set = hasattr(data, "subset") and hasattr(data, "sizes_host")
        lins = [layer.apply_mod.linear for layer in self.layers]
        widths = [lin.out_features for lin in lins]
        if is_set:
            ids = np.asarray(data.ids, dtype=np.int64)
            sizes = data.sizes_host[ids] if len(ids) else np.zeros(0, np.int64)
            feat, mode0 = data.feat, "none"
            n_all = len(data.sizes_host)
            identity_ids = len(ids) == n_all and bool((ids == np.arange(n_all)).all())
        else:
            feat = data.ndata['h']
            if not (isinstance(feat, torch.Tensor) and feat.is_cuda):
                raise ops.GaeHipError(f"GAE.{who}: the HIP path needs device tensors")
            data._follow(feat)
            counts = data.batch_num_nodes if data.batch_num_nodes is not None else [data.number_of_nodes()]
            sizes = np.asarray(counts, dtype=np.int64)
            ids, identity_ids, mode0 = np.arange(len(sizes), dtype=np.int64), True, data.norm_mode
        modes = {mode0 if layer.norm is None else layer.norm for layer in self.layers}
        codes = [_act_code(layer.apply_mod.activation) for layer in self.layers]
        why = None
        if len(modes) != 1 or next(iter(modes)) not in ("none", "both"):
            why = f"norm modes {sorted(map(str, modes))}: one of 'none' / 'both' for all layers"
        elif any(c is None for c in codes):
            why = "an activation that is neither identity nor ReLU"
        elif feat.dtype not in (torch.uint8, torch.float32):
            why = f"{feat.dtype} features (uint8 or fp32)"
        elif not ops.embed_graphs_usable(lins[0].in_features, widths, 0):
            why = f"the encoder {lins[0].in_features} -> {widths}: 1..{ops.EMBED_MAX_LAYERS} layers of widths <= " \
                  f"{ops.EMBED_MAX_WIDTH}"
        return is_set, ids, sizes, identity_ids, feat, next(iter(modes)), codes, why

    def _embed_graphs(self, data, fused, batch_size, grad=False):
        import numpy as np
        is_set, ids, sizes, identity_ids, feat, mode, codes, why = self._graph_set(data, "embed_graphs")
        lins = [layer.apply_mod.linear for layer in self.layers]
        d = lins[-1].out_features
        if grad and why is None and any(p.requires_grad for p in self.parameters()) and \
                not ops.embed_graphs_bwd_usable(lins[0].in_features, [lin.out_features for lin in lins], 0):
            why = f"the encoder {lins[0].in_features} -> {[lin.out_features for lin in lins]} in its backward " \
                  f"(ops.embed_graphs_bwd_usable)"
        if is_set:
            gp, (indptr, indices) = data.graph_ptr, (data.indptr, data.indices)
        dev = feat.device
        B = len(ids)
        take = sizes <= ops.EMBED_MAX_NODES if why is None else np.zeros(B, dtype=bool)
        if fused is True:
            if why is None and not take.all():
                why = f"{int((~take).sum())} graph(s) above {ops.EMBED_MAX_NODES} nodes (largest: {int(sizes.max())})"
            if why is not None:
                raise ops.GaeHipError(f"GAE.embed_graphs(fused=True): the kernel does not take {why}")
        if fused is False:
            take = np.zeros(B, dtype=bool)
        out = None
        n_take = int(take.sum())
        if n_take:
            if n_take == B and identity_ids:
                gids = None
            else:
                gids = torch.from_numpy(np.ascontiguousarray(ids[take])).to(dev)
            if not is_set:
                gp, (indptr, indices) = data.graph_ptr(), data.csr()
            out = ops.embed_graphs(gp, indptr, indices, feat, [lin.weight for lin in lins], [lin.bias for lin in lins],
                                   codes, norm=mode, graph_ids=gids, max_graph_nodes=int(sizes[take].max()))
            if n_take == B:
                return out
        full = torch.empty(B, 3 * d, dtype=torch.float32, device=dev)
        if out is not None:
            full[torch.from_numpy(np.nonzero(take)[0]).to(dev)] = out
        rest = np.nonzero(~take)[0]
        if B == 0:
            return full
        if not is_set:
            # a batched graph is one batch: the existing route embeds all of it, the rows still missing are kept
            from .graph import readout_nodes
            try:
                rows = readout_nodes(data, self.encode(data))
            finally:
                data.ndata['h'] = feat
            if len(rest):
                sel = torch.from_numpy(rest).to(dev)
                full[sel] = rows[sel]
            return full
        from .graph import readout_nodes
        for lo in range(0, len(rest), batch_size):
            sel = rest[lo:lo + batch_size]
            bg = data.batch(ids[sel])
            rows = readout_nodes(bg, self.encode(bg))
            if len(sel) == B:
                return rows
            full[torch.from_numpy(sel).to(dev)] = rows
        return full

    def score_graphs(self, data, *, fused="auto", exclude_self=True, batch_size=4096):
        """``ops.GraphScores(loss, auc, ap, n_pos, n_neg, wins, ties)``, device tensors with one entry per graph of
        ``data`` (the kinds and the order of embed_graphs): how well the encoder reconstructs each molecule -- the
        ROC-AUC and the average precision of z_i . z_j against the molecule's own adjacency over its ordered pairs
        (i != j when ``exclude_self``), the exact counts behind them, and the reference's per-molecule weighted BCE
        (train_inductive.py:44-48) WITHOUT the decoder's dropout.  NaN where a class is missing.
        ``metrics.graph_score_summary`` condenses them.  Runs under no_grad; parameters and ``g.ndata`` are left as
        they were; the norm follows the model as in embed_graphs.
        ``fused=True``: one launch for the whole set (ops.score_graphs: encoder, decoder and ranking per molecule in
        LDS); raises outside the kernel's shapes (1..4 layers, widths <= 64, graphs <= 64 nodes).  ``"auto"``: that
        launch for every graph it takes; a model it does not take runs ``batch`` -> ``encode`` in chunks of
        ``batch_size`` graphs and scores that Z with the kernel's no-layer mode; graphs above 64 nodes are scored one by
        one (metrics.graph_scores_dense).  ``False``: the chunked route for everything."""
        if fused not in ("auto", True, False):
            raise ValueError(f"fused: 'auto', True or False, not {fused!r}")
        if isinstance(batch_size, bool) or int(batch_size) != batch_size or batch_size < 1:
            raise ValueError(f"batch_size: a positive number of graphs, not {batch_size!r}")
        with torch.no_grad():
            return self._score_graphs(data, fused, bool(exclude_self), int(batch_size))

    def _score_graphs(self, data, fused, exclude_self, batch_size):
        import numpy as np
        is_set, ids, sizes, identity_ids, feat, mode, codes, why = self._graph_set(data, "score_graphs")
        lins = [layer.apply_mod.linear for layer in self.layers]
        dev = feat.device
        B = len(ids)
        take = sizes <= ops.EMBED_MAX_NODES if why is None else np.zeros(B, dtype=bool)
        if fused is True:
            if why is None and not take.all():
                why = f"{int((~take).sum())} graph(s) above {ops.EMBED_MAX_NODES} nodes (largest: {int(sizes.max())})"
            if why is not None:
                raise ops.GaeHipError(f"GAE.score_graphs(fused=True): the kernel does not take {why}")
        if fused is False:
            take = np.zeros(B, dtype=bool)
        out = None
        n_take = int(take.sum())
        if n_take:
            if n_take == B and identity_ids:
                gids = None
            else:
                gids = torch.from_numpy(np.ascontiguousarray(ids[take])).to(dev)
            gp, (indptr, indices) = (data.graph_ptr, (data.indptr, data.indices)) if is_set else \
                (data.graph_ptr(), data.csr())
            out = ops.score_graphs(gp, indptr, indices, feat, [lin.weight for lin in lins], [lin.bias for lin in lins],
                                   codes, norm=mode, graph_ids=gids, max_graph_nodes=int(sizes[take].max()),
                                   exclude_self=exclude_self)
            if n_take == B:
                return out
        full = _empty_scores(B, dev)
        if out is not None:
            _put_scores(full, torch.from_numpy(np.nonzero(take)[0]).to(dev), out)
        rest = np.nonzero(~take)[0]
        if not is_set:
            if len(rest):
                # a batched graph is one batch: encode() embeds all of it, the members still missing are scored
                try:
                    z = self.encode(data)
                finally:
                    data.ndata['h'] = feat
                _put_scores(full, torch.from_numpy(rest).to(dev), score_embedding(z, data, exclude_self, members=rest))
            return full
        for lo in range(0, len(rest), batch_size):
            sel = rest[lo:lo + batch_size]
            bg = data.batch(ids[sel])
            _put_scores(full, torch.from_numpy(sel).to(dev), score_embedding(self.encode(bg), bg, exclude_self))
        return full

    def reconstruction_loss(self, g, criterion="bce", scope="batch", samples=None):
        """The training loss of train_inductive.py:44-48 (dense label from g,
        pos_weight, BCE-with-logits mean over all N^2 ordered pairs) evaluated
        by the fused HIP kernel: numerically the same quantity as
        ``BCELoss(self.forward(g), adj, pos_weight)`` without the N x N logits /
        label matrices.  Side effect on ``g.ndata['h']`` as in forward().
        ``criterion="mse"``: the hyper-parameter search's ``nn.MSELoss()(self.forward(g), adj)``
        (optuna_gae.py:16,21), likewise without the N x N matrices (ops.decoder_mse).
        ``scope="graph"``: the same BCE on every member graph of a batched ``g`` alone (its own pairs, pos_weight and
        mean), averaged over the members (ops.decoder_bce_graphs) -- the reference's loss at batch size 1, averaged
        over the molecules of the batch; a graph that is not a batch gives exactly the ``"batch"`` loss.
        ``samples=m``: the unbiased sampled estimate of the BCE loss (ops.decoder_bce_sampled): the edge term exactly,
        the all-pairs term from m keyed-random partners per node, O((E + N m) d) instead of O(N^2 d); the decoder's
        dropout and draw counter as for the exact loss, fresh partners every call.  BCE over the whole batch only."""
        if scope not in ("batch", "graph"):
            raise ValueError(f"scope: 'batch' or 'graph', not {scope!r}")
        if scope == "graph" and criterion != "bce":
            raise ValueError(f"scope='graph' is a BCE loss (criterion 'bce'), not {criterion!r}")
        if samples is not None:
            if criterion != "bce":
                raise ValueError(f"samples: the sampled loss is the BCE loss (criterion 'bce'), not {criterion!r}")
            if scope != "batch":
                raise ValueError("samples: the sampled loss covers the whole batch (scope 'batch'), not 'graph'")
            if isinstance(samples, bool) or int(samples) != samples or samples < 1:
                raise ValueError(f"samples: a positive number of partners per node, not {samples!r}")
        z = g.ndata['h']
        if samples is not None:
            for layer in self.layers:
                z = layer(g, z)
            g.ndata['h'] = z
            return self.decoder.loss_sampled(z, g, int(samples))
        if scope == "graph":
            for layer in self.layers:
                z = layer(g, z)
            g.ndata['h'] = z
            return self.decoder.loss_graphs(z, g)
        if criterion == "mse":
            for layer in self.layers:
                z = layer(g, z)
            g.ndata['h'] = z
            return self.decoder.loss_mse(z, g)
        if criterion != "bce":
            raise ValueError(f"criterion: 'bce' or 'mse', not {criterion!r}")
        for layer in self.layers[:-1]:
            z = layer(g, z)
        # the last layer may run the loss's prepare step in its epilogue (ops.loss_prepare_request)
        with self.decoder.prepare_request(g, z, self.layers[-1].apply_mod.linear.out_features) as req:
            z = self.layers[-1](g, z)
        g.ndata['h'] = z
        return self.decoder.loss(z, g, prepared=req.token)


class InnerProductDecoder(nn.Module):
    """gae.py:63-72.  Dropout is applied regardless of train()/eval() exactly
    like the reference (``F.dropout(z, self.dropout)`` omits ``training=``).
    The mask comes from the library's Philox counter RNG; set ``self.mask`` to
    inject a precomputed multiplier (0 or 1/(1-p)) instead."""

    def __init__(self, activation=torch.sigmoid, dropout=0.1, seed=None):
        super().__init__()
        self.dropout = dropout
        self.activation = activation
        self.mask = None
        self.seed = seed
        self._draws = None       # device-side draw counter (int64[1]); advanced by a device op per forward
        self.last_mask = None

    def _draw_mask(self, z):
        if self.mask is not None:
            return self.mask
        if not self.dropout:
            return None
        seed = self.seed if self.seed is not None else int(torch.initial_seed())
        if self._draws is None or self._draws.device != z.device:
            self._draws = torch.zeros(1, dtype=torch.int64, device=z.device)
        mask = ops.dropout_mask(tuple(z.shape), self.dropout, seed, 0, z.device, draw_counter=self._draws)
        self._draws += 1         # device op: a captured HIP graph draws a fresh mask every replay
        return mask

    def forward(self, z):
        self.last_mask = self._draw_mask(z)
        return self.activation(ops.decoder_dense(z, self.last_mask))

    def _loss_dropout(self, device):
        """(p, seed, offset, draw counter) of a mask drawn inside a launch, or None (given mask / no dropout)"""
        if self.mask is not None or not self.dropout:
            return None
        seed = self.seed if self.seed is not None else int(torch.initial_seed())
        if self._draws is None or self._draws.device != device:
            self._draws = torch.zeros(1, dtype=torch.int64, device=device)
        return (self.dropout, seed, 0, self._draws)

    def prepare_request(self, g, h, d):
        """the request a producer of Z answers by running this loss's prepare step in its own launch"""
        on_gpu = isinstance(h, torch.Tensor) and h.is_cuda
        return ops.loss_prepare_request(g if on_gpu else None, d, self.mask, self._loss_dropout(h.device) if on_gpu else None)

    def loss_mse(self, z, g):
        """nn.MSELoss()(self.forward(z), adj) (optuna_gae.py:16,21; identity activation) without the N x N matrices; the
        dropout mask is drawn as forward() draws it and kept in ``last_mask``"""
        if not (isinstance(z, torch.Tensor) and z.is_cuda):
            raise ops.GaeHipError("InnerProductDecoder.loss_mse: the HIP path needs device tensors")
        self.last_mask = self._draw_mask(z)
        return ops.decoder_mse(z, self.last_mask, g)

    def loss_graphs(self, z, g):
        """the fused loss per member graph of a batched ``g``, averaged over the members (ops.decoder_bce_graphs).  The
        dropout mask is drawn inside the launch (same Philox stream as loss()) and kept in ``last_mask``."""
        if not (isinstance(z, torch.Tensor) and z.is_cuda):
            raise ops.GaeHipError("InnerProductDecoder.loss_graphs: the HIP path needs device tensors")
        drop = self._loss_dropout(z.device)
        if drop is None:
            self.last_mask = self.mask
            return ops.decoder_bce_graphs(z, self.mask, g)
        mask = torch.empty(tuple(z.shape), dtype=torch.float32, device=z.device)
        self.last_mask = mask
        return ops.decoder_bce_graphs(z, mask, g, dropout=drop)

    def loss_sampled(self, z, g, samples):
        """the unbiased sampled estimate of loss() (ops.decoder_bce_sampled) from ``samples`` partners per node.  The
        draw counter advances every call (the partners change), the dropout mask is drawn in the launch as loss() draws
        it and kept in ``last_mask``."""
        if not (isinstance(z, torch.Tensor) and z.is_cuda):
            raise ops.GaeHipError("InnerProductDecoder.loss_sampled: the HIP path needs device tensors")
        seed = self.seed if self.seed is not None else int(torch.initial_seed())
        if self._draws is None or self._draws.device != z.device:
            self._draws = torch.zeros(1, dtype=torch.int64, device=z.device)
        drop = self._loss_dropout(z.device)
        if drop is None:
            self.last_mask = self.mask
            return ops.decoder_bce_sampled(z, self.mask, g, samples, dropout=(0.0, seed, 0, self._draws))
        mask = torch.empty(tuple(z.shape), dtype=torch.float32, device=z.device)
        self.last_mask = mask
        return ops.decoder_bce_sampled(z, mask, g, samples, dropout=drop)

    def loss(self, z, g, prepared=None):
        """fused decoder + weighted BCE (identity activation = logits, gae.py:47).  The dropout mask of this call
        is drawn inside the fused launch (same Philox stream as _draw_mask) and kept in ``last_mask``.
        ``prepared``: the producer of z already ran the prepare step (prepare_request)."""
        if prepared is not None:
            self.last_mask = prepared["mask"]
            return ops.decoder_bce(z, None, g, prepared=prepared)
        drop = self._loss_dropout(z.device)
        if drop is None:
            self.last_mask = self.mask
            return ops.decoder_bce(z, self.mask, g)
        mask = torch.empty(tuple(z.shape), dtype=torch.float32, device=z.device)
        self.last_mask = mask
        return ops.decoder_bce(z, mask, g, dropout=drop)
