"""Variational graph auto-encoder (BASELINE config 5).  The reference only
cites the paper (README.md:58, Kipf & Welling 2016); this follows the paper
with the reference's building blocks: a shared GCN layer (ReLU), two GCN heads
with identity activation for mu and log(sigma), z = mu + eps * exp(log sigma),
loss = weighted BCE reconstruction (the fused decoder+BCE kernel, identical to
GAE's) + KL = -(0.5 / N) * mean_i sum_j (1 + 2 log sigma - mu^2 - sigma^2).

Feature storage may be bf16 (``g.ndata['h']`` in torch.bfloat16): the
layer-1 aggregation then runs the bf16-storage / fp32-accumulate SpMM."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .gae import (_UNSET, GCN, InnerProductDecoder, identity, reconstruct_embedding, reconstruct_threshold,
                  score_embedding)


# mu and log sigma heads as ONE fused launch on the shared aggregate (gae_x_gcn_layer_fused2) and one packed gradient
# path; False runs them as two GCN layers (same values up to the fp32 rounding of the dW summation order)
FUSE_HEADS = True


class VGAE(nn.Module):
    def __init__(self, in_dim, hidden_dims=(32, 16), *, norm=None, seed=None):
        super().__init__()
        h0, d = int(hidden_dims[0]), int(hidden_dims[-1])
        self.shared = GCN(in_dim, h0, F.relu, norm)
        self.mu_head = GCN(h0, d, identity, norm)
        self.logstd_head = GCN(h0, d, identity, norm)
        self.decoder = InnerProductDecoder(activation=identity, dropout=0.0)
        self.seed = seed
        self._draws = None
        self.eps = None          # inject a fixed noise tensor for tests; None = draw from the library RNG
        self.last = {}

    def _heads_packed(self, g, h):
        """[mu | logstd] from ONE fused launch on the shared aggregate (ops.GCNTwoHeadFunction), or None"""
        if not FUSE_HEADS:
            return None
        g._follow(h)
        mode = g.norm_mode if self.mu_head.norm is None else self.mu_head.norm
        if mode not in ("none", "both"):
            return None
        return ops.gcn_two_heads(g, h, self.mu_head.apply_mod.linear, self.logstd_head.apply_mod.linear,
                                 use_norm=(mode == "both"))

    def encode(self, g):
        h = self.shared(g, g.ndata['h'])
        ml = self._heads_packed(g, h)
        if ml is not None:
            d = ml.shape[1] // 2
            return ml[:, :d], ml[:, d:]
        mu = self.mu_head(g, h)
        logstd = self.logstd_head(g, h)
        return mu, logstd

    def _noise(self, like):
        if self.eps is not None:
            return self.eps
        if self._draws is None or self._draws.device != like.device:
            self._draws = torch.zeros(1, dtype=torch.int64, device=like.device)
        seed = self.seed if self.seed is not None else int(torch.initial_seed())
        eps = ops.normal_noise(tuple(like.shape), seed, 0, like.device, draw_counter=self._draws)
        self._draws += 1
        return eps

    def _fused_loss(self, g, ml):
        """head + KL + reconstruction loss as ops.VGAEHeadLossFunction (noise drawn inside its first launch with the
        stream _noise() uses), or None"""
        if self.decoder.dropout or self.decoder.mask is not None or not ml.is_cuda:
            return None
        noise = None
        if self.eps is None:
            if self._draws is None or self._draws.device != ml.device:
                self._draws = torch.zeros(1, dtype=torch.int64, device=ml.device)
            seed = self.seed if self.seed is not None else int(torch.initial_seed())
            noise = (seed, 0, self._draws)
        return ops.vgae_head_loss(ml, g, self.eps, noise)

    def loss(self, g, samples=None):
        """reconstruction BCE (train_inductive.py:44-48 semantics, fused) + KL.  ``samples=m``: the reconstruction term
        is the unbiased sampled estimate (InnerProductDecoder.loss_sampled, m partners per node)"""
        if samples is not None and (isinstance(samples, bool) or int(samples) != samples or samples < 1):
            raise ValueError(f"samples: a positive number of partners per node, not {samples!r}")
        h = self.shared(g, g.ndata['h'])
        ml = self._heads_packed(g, h)
        if ml is not None:                       # both heads in one launch, [mu | logstd] packed end to end
            d = ml.shape[1] // 2
            mu, logstd = ml[:, :d], ml[:, d:]
            fused = self._fused_loss(g, ml) if samples is None else None
            if fused is not None:
                loss, z, kl, rec, eps = fused
                g.ndata['h'] = z
                self.decoder.last_mask = None
                self.last = {"mu": mu, "logstd": logstd, "eps": eps, "z": z, "kl": kl, "rec": rec}
                return loss
            eps = self._noise(mu)
            z, kl = ops.vgae_head_packed(ml, eps)
        else:
            mu = self.mu_head(g, h)
            logstd = self.logstd_head(g, h)
            eps = self._noise(mu)
            z, kl = ops.vgae_head(mu, logstd, eps)
        g.ndata['h'] = z
        rec = self.decoder.loss(z, g) if samples is None else self.decoder.loss_sampled(z, g, int(samples))
        self.last = {"mu": mu, "logstd": logstd, "eps": eps, "z": z, "kl": kl, "rec": rec}
        return rec + kl

    def predict_links(self, g, k, *, scope="batch", exclude_self=True, exclude_edges=True):
        """GAE.predict_links on the mean embedding mu (no noise): the k largest mu_i . mu_j per node among the
        non-edges of ``g`` (ops.decoder_topk)"""
        with torch.no_grad():
            mu, _ = self.encode(g)
        return ops.decoder_topk(mu, k, g, scope=scope, exclude_self=exclude_self, exclude_edges=exclude_edges)

    def rank_links(self, g, pairs, *, filter_graph=None, scope="batch", exclude_self=True, exclude_edges=True):
        """GAE.rank_links on the mean embedding mu (no noise): the filtered rank counts of the pairs (i, j) among all
        candidates of i (ops.decoder_rank)"""
        with torch.no_grad():
            mu, _ = self.encode(g)
        return ops.decoder_rank(mu, pairs, g, filter_graph=filter_graph, scope=scope, exclude_self=exclude_self,
                                exclude_edges=exclude_edges)

    def reconstruct(self, g, *, prob=_UNSET, threshold=None, scope="batch", exclude_self=True, exclude_edges=False,
                    max_pairs=2 ** 27):
        """GAE.reconstruct on the mean embedding mu (no noise): ``ops.DecodedLinks`` of the pairs with
        sigmoid(mu_i . mu_j) >= prob (ops.decoder_threshold); ``g.ndata['h']`` is restored on exit"""
        t = reconstruct_threshold(prob, threshold)
        feat = g.ndata['h']
        with torch.no_grad():
            try:
                mu, _ = self.encode(g)
            finally:
                g.ndata['h'] = feat
        return reconstruct_embedding(mu, g, t, scope, exclude_self, exclude_edges, max_pairs)

    def cluster_nodes(self, g, k, **kw):
        """GAE.cluster_nodes on the mean embedding mu (no noise): ``ops.KMeansResult`` of ops.kmeans; mu is read in
        place where the two heads are packed in one buffer; ``g.ndata['h']`` is restored on exit"""
        feat = g.ndata['h']
        with torch.no_grad():
            try:
                mu, _ = self.encode(g)
            finally:
                g.ndata['h'] = feat
        return ops.kmeans(mu, k, **kw)

    def map_nodes(self, g, **kw):
        """GAE.map_nodes on the mean embedding mu (no noise): ``ops.TSNEResult`` of ops.tsne; mu is read in place where
        the two heads are packed in one buffer; ``g.ndata['h']`` is restored on exit"""
        feat = g.ndata['h']
        with torch.no_grad():
            try:
                mu, _ = self.encode(g)
            finally:
                g.ndata['h'] = feat
        return ops.tsne(mu, **kw)

    def pca_nodes(self, g, k=None, **kw):
        """GAE.pca_nodes on the mean embedding mu (no noise): ``ops.PCAResult`` of ops.pca; mu is read in place where
        the two heads are packed in one buffer; ``g.ndata['h']`` is restored on exit"""
        feat = g.ndata['h']
        with torch.no_grad():
            try:
                mu, _ = self.encode(g)
            finally:
                g.ndata['h'] = feat
        return ops.pca(mu, k, **kw)

    def classify_nodes(self, g, labels, **kw):
        """GAE.classify_nodes on the mean embedding mu (no noise): ``ops.LogRegResult`` of ops.logreg; mu is read in
        place where the two heads are packed in one buffer; ``g.ndata['h']`` is restored on exit"""
        feat = g.ndata['h']
        with torch.no_grad():
            try:
                mu, _ = self.encode(g)
            finally:
                g.ndata['h'] = feat
        return ops.logreg(mu, labels, **kw)

    def nearest_nodes(self, g, k, *, metric="l2"):
        """GAE.nearest_nodes on the mean embedding mu (no noise): ``ops.KNNResult`` of ops.knn, the node itself left
        out; mu is read in place where the two heads are packed in one buffer; ``g.ndata['h']`` is restored on exit"""
        feat = g.ndata['h']
        with torch.no_grad():
            try:
                mu, _ = self.encode(g)
            finally:
                g.ndata['h'] = feat
        return ops.knn(mu, k=k, metric=metric)

    def score_graphs(self, g, *, exclude_self=True):
        """GAE.score_graphs on the mean embedding mu (no noise) of a batched graph ``g``: ``ops.GraphScores`` per member
        graph, mu scored through the no-layer mode of ops.score_graphs (gae.score_embedding)"""
        feat = g.ndata['h']
        with torch.no_grad():
            try:
                mu, _ = self.encode(g)
            finally:
                g.ndata['h'] = feat
        return score_embedding(mu, g, exclude_self)

    def forward(self, g):
        """sampled Z Z^T logits (dense parity / inference path)"""
        mu, logstd = self.encode(g)
        z, _ = ops.vgae_head(mu, logstd, self._noise(mu))
        g.ndata['h'] = z
        return self.decoder(z)
