/* gae_hip_experimental.h -- the SEAMS of libgae_hip.so that its own host mirror (gae_dgl_amd/ops/, capture.py,
 * sparse.py, parallel.py) uses to fuse launches, build plans and defer reductions.  A maintainer who binds the library
 * behind the reference's call sites needs gae_hip.h only; nothing here changes a result -- every entry
 * point is a faster composition of, or a set-up step for, an entry point of gae_hip.h:
 *   gae_x_*                     launch-diet forms of a training step (producer epilogues, partial sums handed to the
 *                               optimiser launch, collate steps that read a device-side cursor)
 *   gae_spmm_plan_* / _ell_build / _csr_blockdiag / _csr_epilogue
 *                               plan construction and the specialised aggregation kernels gae_spmm_csr dispatches to
 *   gae_spx_*, gae_dense_to_csr_*   layer 1 from the non-zeros of constant input features (gae_dgl_amd.SparseFeatures)
 *   gae_linear2_*, gae_gcn2_*   the dense halves of a two-layer encoder on millions of rows (row-sharded RMAT path)
 * and gae_decoder_bce_sampled, an unbiased stochastic estimate of gae_decoder_bce's loss for graphs beyond the N^2 sum,
 * and gae_decoder_rank, the filtered rank of given pairs among all candidates of gae_decoder_topk's rule,
 * and gae_score_graphs, the per-molecule reconstruction scores (AUC counts, average precision, loss) of a resident set,
 * and gae_kmeans_*, node clustering on the device: k-means++ seeding, Lloyd iterations and assignment over an embedding,
 * and gae_knn, the exact k nearest rows of one embedding for every row of another,
 * and gae_ridge_*, ridge regression on a frozen feature: per-fold fp64 moments in one pass, the k-fold CV lambda path,
 * and gae_logreg_*, softmax regression on a frozen feature: every fold x lambda model of a CV call in the same launches,
 * and gae_fingerprint_graphs / gae_tanimoto_knn, circular fingerprints of a resident molecule set and their exact search.
 * Same conventions as gae_hip.h: caller-owned buffers, 0 / negative / hipError_t return codes, asynchronous launches on
 * the stream passed last.  These signatures may change between versions without a GAE_VERSION major bump. */
#ifndef GAE_HIP_EXPERIMENTAL_H
#define GAE_HIP_EXPERIMENTAL_H

#include "gae_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* (from gae_hip.h: graph structure) */
/* gae_batch_select + gae_batch_plan in one launch (the step of a captured HIP graph): ids of batch *cursor_dev of the
 * epoch order -> out_ids, their prefix sums -> out_*_ptr, *cursor_dev += 1. */
int gae_x_batch_plan_next(const int64_t *graph_ptr, const int32_t *ds_indptr, const int32_t *ds_t_indptr,
                        const int64_t *order, int64_t n_order, int64_t *cursor_dev, int64_t n_graphs,
                        int64_t *out_ids, int64_t *out_node_ptr, int64_t *out_edge_ptr, int64_t *out_t_edge_ptr,
                        void *stream);

/* gae_x_batch_plan_next + gae_batch_gather (fixed-capacity form) in ONE launch, for batches of <= 1024 graphs: the ids
 * of batch *cursor_dev of the epoch order, their prefix sums (out_ids [n_graphs], out_node_ptr / out_edge_ptr
 * [n_graphs + 1]) and the gathered, capacity-padded batch; *cursor_dev += 1.  out_counts: int64[4], ZERO before the
 * first call -- [0..2] as gae_batch_gather, [3] is the launch's block ticket (left zero).  The CSR of the batch is
 * used for the transposed structure as well (symmetric datasets: every bond stored in both directions,
 * gae_dgl/prepare_data.py:61-64). */
int gae_x_batch_gather_next(const int64_t *graph_ptr, const int32_t *ds_indptr, const int32_t *ds_indices,
                          const void *ds_feat, int64_t ld_feat, int64_t F, int dtype,
                          const int64_t *order, int64_t n_order, int64_t *cursor_dev, int64_t n_graphs,
                          int64_t *out_ids, int64_t *out_node_ptr, int64_t *out_edge_ptr,
                          int64_t cap_nodes, int64_t cap_edges,
                          int32_t *out_indptr, int32_t *out_indices, void *out_feat, int64_t ld_out,
                          int32_t *out_ell, int32_t ell_width, int64_t *out_counts, void *stream);

/* plan construction on the device (csrc/plan_build.hip): classification of the rows, descriptors, compact tagged
 * ids of the mid rows, XCD-pinned regrouping of the very long rows -- integer work, deterministic (ascending rows, stable
 * partition, stable sort).  Every call synchronises `stream` once to hand counters to the host.
 *   sizes_host[0..6] = {light rows (1 .. threshold edges), mid rows (threshold < d <= pin_degree), their segments, their
 *                       edges, pinned rows (d > pin_degree), their edges, maximum degree};  scratch >= 64 bytes
 *   pin_degree = INT32_MAX: no pinned rows (every row above the threshold is a mid row). */
/* light_desc [n_light][4] (or NULL: no list); heavy_rows, heavy_seg_base [n_mid]; seg_heavy [segments]; seg_desc [segments][4]; mid_ids
 * [mid_edges] or NULL (no compact copy; hot_columns > 0 needs it: the ids of the hot_columns most gathered columns get the
 * tag); vh_rows [n_pinned]; vh_part_ptr [n_pinned + 1].  pinned_host_out[0] = virtual rows NV, [2] = tag threshold. */
/* pinned rows, two calls on the SAME scratch: vh_desc == NULL partitions the ids into vh_cols [pinned_edges], sorts the
 * chunks and reports pinned_host_out[1] = V; the second call fills vh_desc [V][4] and vh_part_pos [NV]. */
int gae_spmm_plan_sizes(const int32_t *indptr, int64_t n_rows, int32_t threshold, int32_t pin_degree, int32_t segment_edges,
                        int64_t *sizes_host, void *scratch, int64_t scratch_bytes, void *stream);

int64_t gae_spmm_plan_scratch_bytes(int64_t n_rows, int64_t n_cols, int64_t n_pinned, int64_t pinned_edges,
                                    int32_t segment_edges);

int gae_spmm_plan_build_rows(const int32_t *indptr, const int32_t *indices, int64_t n_rows, int64_t n_cols,
                             int32_t threshold, int32_t pin_degree, int32_t segment_edges, const int64_t *sizes,
                             int64_t hot_columns, int32_t *light_desc, int32_t *heavy_rows, int32_t *heavy_seg_base,
                             int32_t *seg_heavy, int32_t *seg_desc, int32_t *mid_ids, int32_t *vh_rows,
                             int32_t *vh_part_ptr, void *scratch, int64_t scratch_bytes, int64_t *pinned_host_out,
                             void *stream);

int gae_spmm_plan_build_pinned(const int32_t *indptr, const int32_t *indices, int64_t n_rows, int64_t n_cols,
                               int32_t segment_edges, const int64_t *sizes, const int32_t *vh_rows, int32_t *vh_cols,
                               int32_t *vh_desc, int32_t *vh_part_pos, void *scratch, int64_t scratch_bytes,
                               int64_t *pinned_host_out, void *stream);

/* width: 4, 8 or 16 slots per row */
int gae_spmm_ell_build(const int32_t *indptr, const int32_t *indices, int64_t n_rows, int32_t width,
                       int32_t skip_degree, int32_t *ell, void *stream);

/* Block-diagonal form of the same product (the batched molecule graphs of gae_dgl/train_inductive.py:31-35):
 * block_ptr[n_blocks + 1] (int32, device) cuts the rows into runs that are CLOSED under adjacency (whole member
 * graphs; every column id of a run's rows lies inside the run).  One thread block streams its slice of H into
 * LDS with coalesced 16-byte loads and gathers from there.  fp32, n_cols == n_rows, 16-byte aligned rows
 * (ld % 4 == 0).  max_block_rows bounds a run's row count, max_block_edges the index slice staged in LDS (edges
 * beyond it are read from global memory): gae_spmm_blockdiag_lds_bytes(...) <= 160 KiB.  Same CSR-order sums as
 * gae_spmm_csr (bit-identical results). */
int64_t gae_spmm_blockdiag_lds_bytes(int64_t max_block_rows, int64_t max_block_edges, int64_t ldh);

int gae_spmm_csr_blockdiag(const int32_t *indptr, const int32_t *indices, const int32_t *block_ptr,
                           const int32_t *block_eptr /* [n_blocks + 1] = indptr[block_ptr[.]] */,
                           int64_t n_blocks, int64_t max_block_rows, int64_t max_block_edges, int64_t n_rows,
                           const float *H, int64_t ldh, float *M, int64_t ldm, int64_t F,
                           const float *row_scale, const float *col_scale, int flags, void *stream);

/* (from gae_hip.h: transform-first GCN layer) */
int64_t gae_xw_fwd_splits(int64_t n, int64_t f_in, int64_t f_out, int dtype);

/* The first half of gae_xw_wgrad only: the per-(row partition, column slice) partial products stay in `workspace`
 * (gae_xw_wgrad_workspace_bytes) and layout_out describes them for gae_adam_step's deferred reduction:
 *   layout_out[0] = partials of dW, [1] = floats between two of them, [2] = row pitch (floats) of a partial's [f_out]
 *   rows (element (j, k) of partial q: workspace[q * [1] + j * [2] + k]); [3] = float offset of the db partials,
 *   [4] = their count, [5] = floats between two of them (element j of partial q: workspace[[3] + q * [5] + j]). */
int gae_x_xw_wgrad_partials(const void *X, int64_t ldx, int dtype, int64_t n, int64_t f_in,
                          const float *G, int64_t ldg, const float *Gmask, int64_t ldgm,
                          const float *D, int64_t ldd, const float *Dmask, int64_t lddm, int64_t f_out,
                          int want_dW, int want_db, void *workspace, int64_t workspace_bytes,
                          int64_t *layout_out, void *stream);

int gae_spmm_csr_epilogue(const int32_t *indptr, const int32_t *indices, int64_t n_rows, int64_t n_cols,
                          const float *H, int64_t ldh, const float *Hmask, float *Y, int64_t ldy, int64_t F,
                          const float *row_scale, const float *col_scale, const gae_spmm_plan *plan,
                          const float *bias, int act, int64_t n_splits, int64_t split_stride, void *stream);

/* Two GCN heads on one aggregate in ONE launch (VGAE's mu and log sigma heads, gae_dgl_amd/vgae.py; the reference has
 * a single head: gae_dgl/gae.py:36-45): gae_gcn_layer_fused with the weight given as two matrices stacked along their
 * STORED rows ([W; W2], w_split rows in W, same strides) and the bias as [bias; bias2].  Forward (w_transposed = 0):
 * Y = [act(M W^T + b) | act(M W2^T + b2)].  Backward of identity heads (w_transposed = 1, strides swapped as in
 * gae_gcn_layer_fused): dH = (A^T dY) [W; W2]. */
int gae_x_gcn_layer_fused2(const int32_t *indptr, const int32_t *indices, int64_t n_rows, int64_t n_cols,
                         const float *H, int64_t ldh, float *M, int64_t ldm, int64_t F,
                         const float *row_scale, const float *col_scale, const gae_spmm_plan *plan,
                         const float *W, const float *W2, int64_t w_split, int w_transposed,
                         int64_t w_stride_out, int64_t w_stride_in, const float *bias, const float *bias2,
                         int64_t J, int act, float *Y, int64_t ldy, void *stream);

/* The identity-activation BACKWARD of gae_gcn_layer_fused (gae_dgl/gae.py:26-31 under autograd) in one launch:
 *   dH [n, f_in] (lddh) = (A^T dY) W        the fused kernel on the CSR of A^T (plan_t: its plan), W [f_out, f_in] (ldw)
 *                                            as nn.Linear stores it;
 *   dW [f_out, f_in] = dY^T M,  db [f_out] = colsum(dY)     side work of the same thread blocks on their own 32 (16)
 *                                            rows: M [n, f_in] (ldm) is the aggregate the forward stored.
 * dY [n, f_out] (lddy: whole 16-byte vectors), f_out <= 32, f_in <= 32, square graph.  The weight gradient leaves the
 * launch as per-block partial sums in `workspace` (gae_x_gcn_layer_fused_wgrad_workspace_bytes(n, f_out, f_in)):
 * layout_out[0] = number of partials, [1] = floats between two partials, [2] = float offset of the db partials inside
 * one (dW partial: element o * f_in + i).  dW / db != NULL: a second, small launch adds them up (the library's one
 * order for partial lists); both NULL: the caller hands the list to gae_adam_step (gae_adam_tensor.partials) -- no
 * weight-gradient launch at all in a captured training step. */
int64_t gae_x_gcn_layer_fused_wgrad_workspace_bytes(int64_t n_rows, int64_t f_out, int64_t f_in);

int gae_x_gcn_layer_fused_wgrad(const int32_t *t_indptr, const int32_t *t_indices, int64_t n, const float *dY,
                              int64_t lddy, int64_t f_out, const float *row_scale, const float *col_scale,
                              const gae_spmm_plan *plan_t, const float *W, int64_t ldw, int64_t f_in, float *dH,
                              int64_t lddh, const float *M, int64_t ldm, float *dW, float *db, void *workspace,
                              int64_t workspace_bytes, int64_t *layout_out, void *stream);

/* ... and of gae_x_gcn_layer_fused2 (two identity heads on one aggregate): dY = [dY1 | dY2] ([n, f_out], f_out = d1 + d2),
 * the weight is the stack [W; W2] along its stored rows (w_split = d1 rows come from W; both ldw apart), dW [f_out, f_in]
 * is stacked alike (rows < w_split = dW1), db [f_out]. */
int gae_x_gcn_layer_fused2_wgrad(const int32_t *t_indptr, const int32_t *t_indices, int64_t n, const float *dY,
                               int64_t lddy, int64_t f_out, const float *row_scale, const float *col_scale,
                               const gae_spmm_plan *plan_t, const float *W, const float *W2, int64_t w_split,
                               int64_t ldw, int64_t f_in, float *dH, int64_t lddh, const float *M, int64_t ldm, float *dW,
                               float *db, void *workspace, int64_t workspace_bytes, int64_t *layout_out, void *stream);

/* (from gae_hip.h: dense halves of a two-layer encoder on very tall operands (csrc/tall.hip)) */
/* ---- dense halves of a two-layer encoder on very tall operands (csrc/tall.hip) ---------------------------------
 * gae_linear2_fwd:  Y1 = act1(A W1^T + b1) [n, f_mid],  T = Y1 W2^T [n, f_out]  in ONE pass over A [n, f_in]:
 * NodeApplyModule of layer 1 (gae_dgl/gae.py:13-16) and the dense half of layer 2 evaluated transform-first.
 * f_in <= 64, f_mid <= 32, f_out <= 32; rows of A, Y1, T whole 16-byte vectors; W1 [f_mid, f_in] (ldw1), W2 [f_out,
 * f_mid] (ldw2) as nn.Linear stores them; b1 may be NULL; Y1 may be NULL (inference: only T is wanted). */
/* a_dead [n] (or NULL): rows of A that ARE zero and were never written -- the rows without edges of an aggregate
 * produced with GAE_SPMM_SKIP_ROWS -- are not read (their outputs are act1(b1) and its image under W2).
 * rows [n_listed] (or NULL; replaces a_dead): LIST MODE -- only the listed rows (ascending ids < n) are read, computed
 * and written; the pass is bound by the fp32 matrix pipe, so on a power-law graph, where most rows of an aggregate
 * have no in-edges, it does a fraction of the work.  gae_linear2_fill_dead writes T for all the other rows (their
 * common value act1(b1) W2^T; `dead` [n] marks them). */
/* gae_gcn2_bwd_dense: every dense product of that encoder's backward pass in ONE pass over its four tall operands
 * (train_inductive.py:51 for the model of gae.py:36-45 with two layers), given G = A^T dZ [n, f_out]:
 *     dW2 = G^T Y1,  db2 = colsum(dZ),  dY1 = (G W2) (.) act1'(Y1),  dW1 = dY1^T M1,  db1 = colsum(dY1)
 * Y1 [n, f_mid] = the output of layer 1, M1 [n, f_in] = its stored aggregate A X; widths <= 32; rows of G and dZ whole
 * 16-byte vectors.  dY1 is never stored.  Per-block partial sums go to `workspace` (gae_gcn2_bwd_dense_workspace_bytes)
 * and are added in block order (deterministic).  layout_out != NULL: stop after the partials (dW1 .. db2 are not
 * written) and report {n_partials, floats per partial, offset of db1, of dW2, of db2} (dW1 at 0) for gae_adam_step's
 * deferred reduction. */
/* m1_dead / g_dead [n] (or NULL; recomputing form only): rows of M1 / G that ARE zero and were never written
 * (GAE_SPMM_SKIP_ROWS) are not read.
 * rows [n_listed] (or NULL): LIST MODE -- the rows that HAVE an M1 row, ascending; m1_dead must then mark exactly the
 * others.  The pass visits the listed rows only (g_dead_listed [n_listed]: the G mask by list entry, or NULL); the
 * others' share -- their H1 row is act1(b1), so it is a rank-one term of the column sums of their G and dZ rows --
 * is computed by two small launches and appended to the partial list as one more partial (workspace sized for it). */
/* (Y1 == NULL: the pass RECOMPUTES Y1 = act1(M1 W1^T + b1) from the tile of M1 it reads anyway -- W1 [f_mid, f_in] (ldw1),
 *  b1 [f_mid] or NULL -- with gae_linear2_fwd's products in its order, i.e. the same bits: the forward then need not
 *  store Y1 at all (gae_linear2_fwd with Y1 = NULL) and this pass reads 2 f_mid fewer floats per row.) */

int gae_linear2_fwd(const float *A, int64_t lda, int64_t n, int64_t f_in, const float *W1, int64_t ldw1,
                    const float *b1, int64_t f_mid, int act1, const float *W2, int64_t ldw2, int64_t f_out,
                    float *Y1, int64_t ldy1, float *T, int64_t ldt, const uint8_t *a_dead, const int32_t *rows,
                    int64_t n_listed, void *stream);

int gae_linear2_fill_dead(const float *b1, int64_t f_mid, int act1, const float *W2, int64_t ldw2, int64_t f_out,
                          const uint8_t *dead, int64_t n, float *T, int64_t ldt, void *stream);

int64_t gae_gcn2_bwd_dense_workspace_bytes(int64_t n, int64_t f_in, int64_t f_mid, int64_t f_out);

int gae_gcn2_bwd_dense(const float *G, int64_t ldg, const float *dZ, int64_t lddz, const float *Y1, int64_t ldy1,
                       int act1, const float *M1, int64_t ldm1, const float *W2, int64_t ldw2, int64_t n,
                       int64_t f_in, int64_t f_mid, int64_t f_out, float *dW1, float *db1, float *dW2, float *db2,
                       void *workspace, int64_t workspace_bytes, int64_t *layout_out, const float *W1, int64_t ldw1,
                       const float *b1, const uint8_t *m1_dead, const uint8_t *g_dead, const int32_t *rows,
                       int64_t n_listed, const uint8_t *g_dead_listed, void *stream);

/* (from gae_hip.h: layer 1 on SPARSE input features (opt-in; gae_dgl_amd.SparseFeatures)) */
/* ---- layer 1 on SPARSE input features (opt-in; gae_dgl_amd.SparseFeatures) -------
 * The citation features the reference loads as a dense FloatTensor (gae_dgl/train_transductive.py:37-38) are
 * bag-of-words rows with 1-10 % non-zeros.  Handed over in compressed form they give the same layer-1 values
 * (the skipped terms are exact zeros) from 8 bytes per non-zero instead of 4 bytes per entry:
 *   gae_dense_to_csr_count / _fill: compressed rows of a dense [n, K] matrix, columns ascending (count the non-zeros
 *       per row, prefix-sum them on the caller's side into rowptr[n + 1], fill col / val); used for X and for X^T.
 *   gae_spx_fwd:   P [n, f_out] = X W^T from the compressed rows of X (f_out <= 32), ascending-column order; the weight
 *       is first transposed into `workspace` (gae_spx_fwd_workspace_bytes(f_in): f_in rows of one 128-byte line), so that a
 *       non-zero gathers ONE line.  Measured (tools/r04/spx_bench.py, pair fwd + wgrad against gae_xw_fwd + gae_xw_wgrad):
 *       Citeseer 17.5 vs 34.7 us, Cora 15.0 vs 16.8 us, Pubmed 27.7 vs 26.4 us -- worth it for wide, very sparse X only
 *       (SparseFeatures.maybe_from_dense applies that rule).
 *   gae_spx_wgrad: dW [f_out, f_in] = G^T X from the compressed rows of X^T cut into SEGMENTS of <= 64 entries of
 *       one feature (seg_feat / seg_e0 / seg_slot [n_segments]: feature, first entry, index of the segment inside its
 *       feature; every feature has at least one -- possibly empty -- segment), and db = colsum(D (.) [Dmask > 0]).
 *       reduce = 1: dW / db are finished by a second launch; reduce = 0: the partial lists stay in `workspace`
 *       (gae_spx_wgrad_layout: [0] partials per element of dW, [1] floats between them (element (j, k) at j * f_in + k),
 *       [2] float offset of the db partials, [3] their count (32 floats apart), [4] workspace bytes) for
 *       gae_adam_step's deferred reduction. */

int gae_dense_to_csr_count(const float *X, int64_t ldx, int64_t n, int64_t K, int32_t *row_nnz, void *stream);

int gae_dense_to_csr_fill(const float *X, int64_t ldx, int64_t n, int64_t K, const int32_t *rowptr, int32_t *col,
                          float *val, void *stream);

int64_t gae_spx_fwd_workspace_bytes(int64_t f_in);

int gae_spx_fwd(const int32_t *rowptr, const int32_t *col, const float *val, int64_t n, int64_t f_in,
                const float *W, int64_t ldw, int64_t f_out, float *P, int64_t ldp, void *workspace,
                int64_t workspace_bytes, void *stream);

int gae_spx_wgrad_layout(int64_t n, int64_t f_in, int64_t max_segments_per_feature, int64_t *out);

int gae_spx_wgrad(const int32_t *t_rowptr, const int32_t *t_row, const float *t_val,
                  const int32_t *seg_feat, const int32_t *seg_e0, const int32_t *seg_slot, int64_t n_segments,
                  int64_t max_segments_per_feature, int64_t n, int64_t f_in,
                  const float *G, int64_t ldg, const float *D, int64_t ldd, const float *Dmask, int64_t lddm,
                  int64_t f_out, float *dW, int64_t lddw, float *db, int reduce,
                  void *workspace, int64_t workspace_bytes, void *stream);

/* (from gae_hip.h: K3-K5: node-apply (Linear + activation)) */
/* The first half of gae_linear_bwd's (dW, db): the per-row-slot partial products stay in `workspace` for
 * gae_adam_step's deferred reduction.  layout_out[0] = slots, [1] = floats between two slots (element e = o * f_in + i
 * of slot q: workspace[q * [1] + e]), [2] = float offset of a slot's f_out column sums (db) inside the slot. */
int gae_x_linear_bwd_partials(const float *dY, int64_t lddy, const float *Y, int64_t ldy, int act,
                            const float *M, int64_t ldm, int64_t n, int64_t f_in, int64_t f_out,
                            int want_dW, int want_db, void *workspace, int64_t workspace_bytes,
                            int64_t *layout_out, void *stream);

/* (from gae_hip.h: K7+K8+K9 fused: decoder + weighted BCE-with-logits, never materialising N x N) */
int gae_x_decoder_bce_prep_layout(int64_t n, int64_t d, void *workspace, int64_t workspace_bytes, gae_bce_prep *out);

/* gae_gcn_layer_fused (identity activation, square graph, J <= 16 outputs = the embedding Z [n, J], ldz) + the prepare
 * work of the loss that follows: mask [n, J] (ldmask) is the dropout multiplier -- drawn here (dropout_p > 0: the
 * Philox stream of gae_dropout_mask with *draw_dev as the draw index, written to `mask`) or given (dropout_p == 0, mask
 * may be NULL = all ones); counts_dev != NULL: fixed-capacity batch, rows >= counts_dev[0] are padding.
 * *n_prep_blocks_out = the number of column-sum partials written (pass it to gae_x_decoder_bce_prepared). */
int gae_x_gcn_layer_fused_prep(const int32_t *indptr, const int32_t *indices, int64_t n, const float *H, int64_t ldh,
                             float *M, int64_t ldm, int64_t F, const float *row_scale, const float *col_scale,
                             const gae_spmm_plan *plan, const float *W, int64_t w_stride_out, int64_t w_stride_in,
                             const float *bias, int64_t J, float *Z, int64_t ldz, const gae_bce_prep *prep, float *mask,
                             int64_t ldmask, float dropout_p, uint64_t seed, uint64_t offset, const uint64_t *draw_dev,
                             const int64_t *counts_dev, int64_t *n_prep_blocks_out, void *stream);

int gae_x_decoder_bce_prepared(float *mask, int64_t ldz, int64_t n, int64_t d, const int32_t *indptr,
                             const int32_t *indices, const int32_t *t_indptr, const int32_t *t_indices,
                             float pos_weight, const int64_t *counts_dev, float dropout_p, uint64_t *draw_dev,
                             int64_t n_prep_blocks, float *loss_out, float *dZ, int64_t lddz, void *workspace,
                             int64_t workspace_bytes, void *stream);

/* The VGAE head AND everything between it and the dense kernel of the loss in one launch (d = 16): eps of this draw
 * (draw_eps != 0: generated with gae_normal_noise's stream -- seed, offset, *draw_dev -- and WRITTEN to eps [n, d];
 * draw_eps == 0: eps is read), z = mu + eps exp(logstd) [n, d], the KL term as one partial per block of 64 rows in
 * kl_partial (capacity kl_capacity >= ceil(n / 64) doubles; scale -0.5 / n^2: put both into gae_bce_tail::kl_*), and
 * the prepare step of gae_decoder_bce on z without dropout (prep: gae_x_decoder_bce_prep_layout; then
 * gae_x_decoder_bce_prepared with *n_blocks_out).  mu / logstd: rows ldm floats apart (packed [mu | logstd]: ldm = 2 d). */
int gae_x_vgae_head_prep(const float *mu, const float *logstd, int64_t ldm, float *eps, int draw_eps, uint64_t seed,
                       uint64_t offset, const uint64_t *draw_dev, int64_t n, int64_t d, float *z, const gae_bce_prep *prep,
                       double *kl_partial, int64_t kl_capacity, int64_t *n_blocks_out, void *stream);

/* (from gae_hip.h: K7+K8+K9, the fused loss) */
/* ---- K17: unbiased sampled estimate of gae_decoder_bce's loss, O((E + n_local m) d) per call
 * The loss of gae_decoder_bce splits exactly (sp = softplus, x_ij = zt_i . zt_j, Zt = Z (.) mask, y_ij = #edges j->i,
 * pw = pos_weight):
 *   L = (1/N^2) [ sum_{all i,j} sp(x_ij) + sum_{edges e=(i,j)} (pw sp(-x_e) - sp(x_e)) ]
 * For the rows r in [row_begin, row_begin + n_local) and m in [1, N] samples per row this call returns
 *   Lhat = (1/N^2) [ (N/m) sum_r sum_{s<m} sp(x_{r,pi_s(r)}) + sum_{edges (r,j) in the rows} (pw sp(-x_rj) - sp(x_rj)) ]
 * and dZ = d Lhat / d Z exactly (the mask included).  E[Lhat] = L (each partner is uniform over [0, N)); at m = N every
 * pair appears once and Lhat = L up to rounding.
 * SAMPLER of draw t = offset + *draw_dev (0 when draw_dev is NULL):
 *   keys      philox4x32_10(counter = 0 | 1, draw = t, key = seed ^ 0xD1B54A32D192ED03) -> words k0..k3 of sigma | tau
 *             (a stream of its own: the dropout mask uses key = seed)
 *   domain    b = smallest integer with 2^b >= N; h = b >> 1; widths (wl, wr) = (b - h, h)
 *   F(R, k)   x = R ^ k; x *= 0x9E3779B1; x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13   (uint32 arithmetic)
 *   E(v)      4 rounds q = 0..3: L = v >> wr, R = v & (2^wr - 1), v = (R << wl) | (L ^ (F(R, k_q) & (2^wl - 1))),
 *             then swap(wl, wr): a bijection of [0, 2^b)
 *   perm(i)   v = E(i); while v >= N: v = E(v)         (cycle walking: a bijection of [0, N)); perm^-1 walks E^-1
 *   o_s       = tau(s), s < m                            (m distinct offsets)
 *   pi_s(i)   = sigma^-1((sigma(i) + o_s) mod N)         (a bijection for every s; row i gets m distinct partners)
 *   the partner of column j in slot s is i = sigma^-1((sigma(j) - o_s) mod N): a gather, no scatter, no atomics.
 * Every local row owns its gradient row and sums, in this order: its edges (CSR of A), its transposed edges (CSR of
 * A^T), its m samples, its m inverse partners.  dZ has the same bits whatever the grid and the row partition; the loss
 * is an ordered fp64 reduction (deterministic run to run).
 *   Z / mask     the full [n, d] arrays (ld ldz); d <= 64.  dropout_p > 0: the mask of this draw is drawn in the launch
 *                (the stream of gae_dropout_mask / gae_decoder_bce at *draw_dev) and written to mask; dropout_p == 0:
 *                mask is an optional input
 *   CSRs         the local row blocks (n_local + 1 entries) with global column ids, as gae_decoder_bce_rows; the CSR
 *                of A^T is required iff dZ != NULL
 *   loss_out     this block's share of Lhat (1 fp32; the shares of a row partition sum to Lhat)
 *   dZ           [n_local, d] (ld lddz), NULL = loss only
 *   partners_out int32 [n_local, m] (may be NULL): pi_s(r) (tests, diagnosis)
 *   draw_dev     device uint64, may be NULL: *draw_dev += 1 once per call, also without dropout, so a replayed HIP
 *                graph draws fresh pairs every time
 *   workspace    NULL = size query: *workspace_bytes receives the bytes needed and nothing else happens (no device
 *                work; works without a GPU).  Otherwise *workspace_bytes is the capacity given.  O(n d + n_local) bytes.
 * Argument errors are returned before any launch: n, d <= 0, n_local or row_begin negative, the row window outside
 * [0, n), d > 64, m outside [1, n], dropout_p outside [0, 1), dZ without the CSR of A^T. */
int gae_decoder_bce_sampled(const float *Z, float *mask, int64_t ldz, int64_t n, int64_t d, int64_t row_begin,
                            int64_t n_local, int64_t m, const int32_t *indptr, const int32_t *indices,
                            const int32_t *t_indptr, const int32_t *t_indices, float pos_weight, float dropout_p,
                            uint64_t seed, uint64_t offset, uint64_t *draw_dev, float *loss_out, float *dZ,
                            int64_t lddz, int32_t *partners_out, void *workspace, int64_t *workspace_bytes,
                            void *stream);

/* (from gae_hip.h: K16, top-k link prediction) */
/* ---- K18: filtered link ranking without the N x N matrix (GAE.rank_links, ops.decoder_rank, metrics.rank_metrics)
 * For query q with i = src[q], j = dst[q] and the threshold t = s_ij = z_i . z_j: where j stands among ALL candidates
 * of row i -- the filtered ranking protocol (MRR, Hits@K for any K, mean rank, the exact all-negatives AUC) that
 * train_transductive.py:35's "# TODO: train test split" needs to say how good a link predictor is.
 * s_ic is the SAME fp32 number gae_decoder_topk computes for that pair and that d: the fp32 MFMA chain in K16's fixed
 * feature order, a function of the bits of z_i and z_c only.  t is produced by the same instruction, never by a second
 * route, so the counts below are defined by equality of bits.
 * Candidates C(i): exactly K16's -- c in i's column window (all n, or i's member [node_ptr[g], node_ptr[g + 1])),
 *   c != i                                 when flags & GAE_TOPK_EXCLUDE_SELF,
 *   c not in CSR row i (indices in any order, repeats counted once)   when flags & GAE_TOPK_EXCLUDE_EDGES,
 *   s_ic neither NaN nor -inf.             Same flags values as gae_decoder_topk.
 * Output, one entry per query:
 *   score_out[q]      = t                                          (fp32)
 *   greater_out[q]    = |{c in C(i) \ {j} : s_ic >  t}|            (int64)
 *   equal_out[q]      = |{c in C(i) \ {j} : s_ic == t}|
 *   candidates_out[q] = |C(i) \ {j}|
 * The target is never counted against itself and NEED NOT be a candidate: it may sit in CSR row i, be i itself or lie
 * outside i's window.  A caller can therefore filter with the full graph, held-out edges included, and still rank each
 * of them.  rank = 1 + greater + equal / 2 (ties share the mean rank).
 *   t NaN                      : greater = candidates, equal = 0 (worst rank); t = +-inf needs no special case
 *   src[q] or dst[q] outside [0, n) : score = NaN, the three counts -1; nothing outside Z is read
 * Several queries may share a source; any order; m = 0 and n = 0 are valid.  1 <= d <= 256, n < 2^31, m < 2^31.
 * Results are integers and one fp32 per query: bit-identical run to run and under any column split.
 *   src / dst    : int64 [m] on the device
 *   node_ptr, max_graph_nodes, indptr / indices : as gae_decoder_topk
 *   workspace    : NULL = size query: *workspace_bytes receives the bytes needed and nothing else happens (no device
 *                  work; works without a GPU).  Otherwise *workspace_bytes is the capacity given.  O(m column splits)
 *                  bytes, never O(m n) or O(n^2).  No logit is written to memory.
 * Cost: the m x n products of the sweep plus, under GAE_TOPK_EXCLUDE_EDGES, one product per CSR entry of the queried
 * rows; the first-occurrence test of a repeated entry is O(1) in a sorted CSR row and O(degree) in an unsorted one.
 * Tuning knob (gae_tuning_set, bit-identical results): "rank_splits" = 0 {0 .. 16}: column splits per panel of 32
 * queries, 0 = auto (the twin of "topk_splits").
 * Argument errors are returned before any launch: d outside 1..256, negative n / m, n or m >= 2^31, ldz < d, unknown
 * flag bits, NULL Z (n > 0), NULL src / dst / output (m > 0), GAE_TOPK_EXCLUDE_EDGES without a CSR, a short workspace.
 * One launch (two when the columns are split over several blocks). */
int gae_decoder_rank(const float *Z, int64_t ldz, int64_t n, int64_t d,
                     const int64_t *src, const int64_t *dst, int64_t m,
                     const int64_t *node_ptr, int64_t n_graphs, int64_t max_graph_nodes,
                     const int32_t *indptr, const int32_t *indices, int flags,
                     float *score_out, int64_t *greater_out, int64_t *equal_out, int64_t *candidates_out,
                     void *workspace, int64_t *workspace_bytes, void *stream);

/* ---- K22: the decoded graph without the N x N matrix (GAE.reconstruct, ops.decoder_threshold)
 * The reconstruction A_hat = 1[sigmoid(z_i . z_j) >= p] of gae.py:69-72 as a CSR: row i lists, in ascending column
 * order, every candidate c of row i with s_ic >= threshold (threshold = log(p / (1 - p)); fp32 compare, a score equal
 * to the threshold is listed), and its score.  s_ic is the SAME fp32 number gae_decoder_topk and gae_decoder_rank
 * compute for that pair and that d (csrc/decoder_pairs.h).
 * Candidates C(i): exactly K16's -- c in i's column window (all n, or i's member [node_ptr[g], node_ptr[g + 1])),
 *   c != i                                 when flags & GAE_TOPK_EXCLUDE_SELF,
 *   c not in CSR row i (indices in any order, repeats allowed)   when flags & GAE_TOPK_EXCLUDE_EDGES,
 *   s_ic neither NaN nor -inf.             Same flags values as gae_decoder_topk.
 * threshold = -inf lists every candidate, +inf only the scores that are +inf; NaN is an argument error.
 * Two calls with the SAME selection arguments (Z .. splits):
 *   gae_decoder_threshold_count  counts the listed pairs of every row and writes row_ptr_out, int64 [n + 1] on the
 *       device: row i's pairs are entries [row_ptr_out[i], row_ptr_out[i + 1]), row_ptr_out[n] is the total (it may
 *       exceed 2^31).  The caller reads the total and allocates.
 *   gae_decoder_threshold_fill   writes index_out int32 [capacity] (the columns) and score_out fp32 [capacity].  It
 *       takes the workspace gae_decoder_threshold_count left behind, UNTOUCHED: that workspace holds the offsets of
 *       every (row, column split), finer than row_ptr, and is what places a pair; row_ptr (as written by _count) is the
 *       array the caller indexes the output by.  Every store is guarded by its position < capacity: too small a
 *       buffer loses the tail of the list and nothing is written outside it.
 * The layout is a function of the scores alone -- no atomic decides a position, no block waits on another --, so every
 * run, schedule and value of `splits` gives the same bytes.
 *   splits       column splits per panel of 32 rows: 0 = auto, else 1 .. 16.  An argument, not a tuning knob; both calls
 *                must be given the same value
 *   node_ptr, max_graph_nodes, indptr / indices : as gae_decoder_topk.  A bad node_ptr never reads outside Z
 *   workspace    : NULL = size query (either call; the same number): *workspace_bytes receives the bytes needed and
 *                  nothing else happens (no device work; works without a GPU).  Otherwise *workspace_bytes is the
 *                  capacity given.  O(n splits) bytes, never O(n^2) and never O(output).  No logit below the
 *                  threshold is written to memory.
 * 1 <= d <= 256, n < 2^31; n = 0 is valid (row_ptr_out[0] = 0).
 * Argument errors are returned before any launch: NaN threshold, splits outside 0..16, d outside 1..256 (GAE_E_RANGE),
 * negative n, n >= 2^31, ldz < d, negative capacity (GAE_E_SIZE), unknown flag bits, NULL Z (n > 0), NULL row_ptr_out /
 * row_ptr, NULL index_out / score_out (capacity > 0), GAE_TOPK_EXCLUDE_EDGES without a CSR, a short workspace.
 * _count: the sweep, then three launches of the prefix sum.  _fill: one launch. */
int gae_decoder_threshold_count(const float *Z, int64_t ldz, int64_t n, int64_t d, float threshold,
                                const int64_t *node_ptr, int64_t n_graphs, int64_t max_graph_nodes,
                                const int32_t *indptr, const int32_t *indices, int flags, int64_t splits,
                                int64_t *row_ptr_out, void *workspace, int64_t *workspace_bytes, void *stream);

int gae_decoder_threshold_fill(const float *Z, int64_t ldz, int64_t n, int64_t d, float threshold,
                               const int64_t *node_ptr, int64_t n_graphs, int64_t max_graph_nodes,
                               const int32_t *indptr, const int32_t *indices, int flags, int64_t splits,
                               const int64_t *row_ptr, int32_t *index_out, float *score_out, int64_t capacity,
                               void *workspace, int64_t *workspace_bytes, void *stream);

/* (from gae_hip.h: graph-level readout) */
/* ---- K19: the molecule feature of a whole resident set in ONE launch (GAE.embed_graphs, ops.embed_graphs)
 * For every selected member graph: the complete GCN encoder of gae.py:26-31,36-45 on that graph's own rows -- per layer
 * aggregate over in-edges, Linear + bias, activation -- followed by gae_segment_readout's [mean | sum | max] over its
 * nodes.  The node embeddings never reach memory.  Every array is read in the layout a resident dataset holds; nothing
 * is copied or re-batched.
 *   graph_ptr    int64 [n_graphs + 1] node offsets of the member graphs; n_nodes rows in all
 *   indptr / indices   int32 CSR of the whole set (rows = destination, GLOBAL column ids, n_edges entries, repeated
 *                entries add); every entry of a row lies inside the row's own member graph
 *   feat         feat_dtype GAE_U8: [n_nodes, ldf] bytes; GAE_F32: [n_nodes, ldf] floats; f_in columns are data, the rest of
 *                a row is padding that is never used as data (it may hold anything, NaN included).  Rows are read with
 *                16-byte loads: feat and the row pitch must be multiples of 16 bytes and hold whole vectors
 *                (ldf >= f_in rounded up to 16 bytes), else GAE_E_ALIGN / GAE_E_SIZE
 *   layers       HOST arrays of n_layers entries: widths[l] = output width of layer l, weights[l] = device pointer to
 *                [widths[l], input width] row-major with leading dimension ldw[l], biases[l] (biases or an entry may be
 *                NULL = no bias), acts[l] = GAE_ACT_IDENTITY / GAE_ACT_RELU (GAE: ReLU on all but the last layer)
 *   norm         GAE_EMBED_NORM_NONE: plain in-edge sums (the reference); GAE_EMBED_NORM_BOTH: D^-1/2 A D^-1/2 with
 *                in_degree^-1/2 (inf -> 0; gae_degree_norm's vector, taken here from the row lengths) as row AND column
 *                scale of every layer
 *   graph_ids    int64 [n_out] on the device, or NULL = graphs 0 .. n_out - 1 (n_out <= n_graphs is the caller's
 *                business): output row k belongs to graph graph_ids[k]; any order, repeats allowed
 *   out          fp32 [n_out, ldo], ldo >= 3 d (d = widths[n_layers - 1]): [mean | sum | max]; an empty graph gives
 *                zeros in all three, as gae_segment_readout
 *   max_graph_nodes   host-side upper bound of the node counts of the selected graphs
 * SHAPES TAKEN: 1 <= n_layers <= 4, f_in and every width in 1..64, max_graph_nodes <= 64 (rows of any length: the
 * neighbour walk follows the CSR).  Anything else returns GAE_E_RANGE, with a message naming the quantity, before any
 * launch; gae_embed_graphs_usable answers the same question (1 = taken) without a launch or a GPU.
 * INDEPENDENCE: a graph's output row is a function of that graph's rows alone -- aggregation sums in CSR order, every
 * product is one fp32 fmaf chain in ascending feature order, the readout adds the graph's nodes first to last.  The
 * row has the same bits whether the graph is embedded with the whole set, in any subset, at any position of graph_ids,
 * twice in one call, or in another run.  No atomics.
 * NUMERICAL CONTRACT: fp32 throughout (products as exact as v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain); within the
 * library's 1e-5 of an fp64 evaluation, measured as everywhere against max(1, max |reference|).
 * ROBUSTNESS: a graph id outside [0, n_graphs), a node range outside [0, n_nodes] or longer than 64 rows (a wrong
 * max_graph_nodes) gives a row of NaN; a row pointer outside [0, n_edges] reads as an empty row; a column id outside
 * the row's own graph is skipped.  Nothing outside the arrays is read or written.
 * Argument errors are returned before any launch: NULL widths / weights / ldw / acts / a layer's weight (GAE_E_NULL),
 * negative sizes, ldo < 3 d, ldw below the input width, short feature rows (GAE_E_SIZE), unknown norm (GAE_E_RANGE),
 * unknown activation or feature dtype (GAE_E_DTYPE), then, when n_out > 0, NULL arrays.  One launch, no workspace. */
enum { GAE_EMBED_NORM_NONE = 0, GAE_EMBED_NORM_BOTH = 1 };

int gae_embed_graphs_usable(int64_t f_in, int64_t n_layers, const int64_t *widths, int64_t max_graph_nodes);

int gae_embed_graphs(const int64_t *graph_ptr, int64_t n_graphs, int64_t n_nodes, int64_t n_edges,
                     int64_t max_graph_nodes, const int32_t *indptr, const int32_t *indices,
                     const void *feat, int feat_dtype, int64_t ldf, int64_t f_in, int64_t n_layers,
                     const int64_t *widths, const float *const *weights, const int64_t *ldw,
                     const float *const *biases, const int *acts, int norm, const int64_t *graph_ids,
                     int64_t n_out, float *out, int64_t ldo, void *stream);

/* ---- K21: the backward of K19 (ops.embed_graphs under autograd, GAE.embed_graphs(grad=True)) in ONE launch plus the
 * reduction of its partials.  Arguments up to n_out: exactly those of the forward entry above (the same arrays, the same
 * checks, the same robustness rules).  Then:
 *   d_out        fp32 [n_out, ldd], ldd >= 3 d: the gradient of a loss with respect to the feature rows
 *   dW, lddw, db HOST arrays of n_layers entries.  dW[l] = device pointer to fp32 [widths[l], input width] with leading
 *                dimension lddw[l], db[l] = device pointer to fp32 [widths[l]]; an ENTRY may be NULL: that gradient is
 *                not wanted (layers below the lowest wanted one are not walked).  Written, not accumulated.  No gradient
 *                with respect to the input features is produced
 *   workspace    device memory of the size the workspace query returns (a pure host function of the shapes and n_out, > 0
 *                and growing with n_out): one partial per parameter and wave
 * Per group of <= 64 rows the encoder runs again in LDS with every layer's aggregated input M_l kept there and the ReLU
 * pass masks as one 64-bit word per lane; nothing per node is saved between the two calls.  Readout:
 * dZ[r][c] = d_sum[c] + d_mean[c] / n + (r == r* ? d_max[c] : 0), r* = the LOWEST row of the graph whose value equals
 * the column's maximum; an empty graph and a refused slot (bad id, bad range, more than 64 rows: the forward's NaN row)
 * contribute nothing.  Per layer, last to first: dY = dH (.) mask, db += sum_r dY[r], dW += dY^T M_l on
 * v_mfma_f32_32x32x2_f32 (accumulators in registers across all groups of a wave), dM = dY W_l, dH = A^T dM as a gather
 * in ascending row order with multiplicities (directed sets, repeated edges, self loops).  No float atomics; the partials
 * are added in the library's one order for such lists: the same call gives the same bits, run to run, and a layer's
 * gradient has the same bits whichever other gradients are asked for.
 * NUMERICAL CONTRACT: fp32 throughout; within the library's 1e-5 of an fp64 evaluation (max |difference| over
 * max(1, max |reference|)).
 * SHAPES TAKEN: the forward's, as far as every M_l, two row buffers and the weights in both orientations fit 160 KB of
 * LDS with one wave and the 32 x 32 accumulator tiles of all layers number at most 8: the usable query below is the
 * truth (1 = taken; no launch, no GPU).  It takes 39->32->16, 39->16, 39->64->32->16 and 39->32->32->32->8 at 64 nodes
 * per graph and refuses e.g. four layers of width 64.  Refusals return GAE_E_RANGE with a message naming the quantity.
 * Argument errors are returned before any launch, as the forward's, plus: NULL dW / lddw / db table (GAE_E_NULL), lddw
 * below the input width, ldd < 3 d, a workspace that is NULL or too small (GAE_E_SIZE).  n_out = 0: nothing is launched,
 * the gradients asked for are set to zero (none asked for: no GPU is needed). */
int gae_embed_graphs_bwd_usable(int64_t f_in, int64_t n_layers, const int64_t *widths, int64_t max_graph_nodes);

int64_t gae_embed_graphs_bwd_workspace_bytes(int64_t f_in, int64_t n_layers, const int64_t *widths, int64_t n_out);

int gae_embed_graphs_bwd(const int64_t *graph_ptr, int64_t n_graphs, int64_t n_nodes, int64_t n_edges,
                         int64_t max_graph_nodes, const int32_t *indptr, const int32_t *indices,
                         const void *feat, int feat_dtype, int64_t ldf, int64_t f_in, int64_t n_layers,
                         const int64_t *widths, const float *const *weights, const int64_t *ldw,
                         const float *const *biases, const int *acts, int norm, const int64_t *graph_ids,
                         int64_t n_out, const float *d_out, int64_t ldd, float *const *dW, const int64_t *lddw,
                         float *const *db, void *workspace, int64_t workspace_bytes, void *stream);

/* The gradient of the segment readout of gae_hip.h (mean | sum | max per member graph) for the chunked route
 * batch -> encode -> readout_nodes: dZ[r][c] = d_sum[c] + d_mean[c] / n + (r == r* ? d_max[c] : 0) for the rows r of
 * graph g (n of them), d_mean / d_sum / d_max = the three blocks of row g of d_out [n_graphs, ldd >= 3 d]; r* = the
 * LOWEST row of the graph whose value of Z equals the column's maximum (K21's tie rule).  Every row of dZ [n_nodes, lddz]
 * that belongs to a graph is written (an empty graph has none).  One wave per graph like the forward, any d (d > 64:
 * column blocks of 64); HBM-bound; no atomics, deterministic. */
int gae_segment_readout_bwd(const float *Z, int64_t ldz, int64_t n_nodes, int64_t d, const int64_t *graph_ptr,
                            int64_t n_graphs, const float *d_out, int64_t ldd, float *dZ, int64_t lddz, void *stream);

/* ---- K20: how well a molecule set is reconstructed, per graph, in ONE launch (GAE.score_graphs, ops.score_graphs)
 * K19's pipeline with a second tail: for every selected member graph the same encoder on the graph's own rows (the Z
 * that is ranked has the bits of the Z gae_embed_graphs reads out), then the inner-product decoder on the graph's own
 * ordered pairs, ranked and scored in LDS.  Nothing of width n_nodes and nothing of size n^2 reaches memory.
 * Arguments up to n_out: exactly gae_embed_graphs's, with one more mode: n_layers = 0 takes the fp32 feature rows AS
 * the embedding Z (f_in = its width, 1..64; feat_dtype must be GAE_F32; widths .. acts may be NULL) -- a Z produced by
 * any other route (VGAE's mu, a wide model) is scored through it.
 * For graph g with rows [r0, r0 + n):
 *   logits     s_ij = the fmaf chain over k = 0 .. d-1 ascending, from 0.f, of z_i[k] z_j[k]; no dropout.  A function of
 *              the bits of z_i and z_j only; s_ij == s_ji bit for bit
 *   pairs      the ordered pairs (i, j) of the graph, i != j when exclude_self = 1.  (i, j) is a POSITIVE iff column
 *              r0 + j occurs in CSR row r0 + i (a repeated entry counts once; columns outside the graph's own rows are
 *              ignored); every other pair is a NEGATIVE
 *   counts_out int64 [n_out][4] = n_pos, n_neg, wins, ties: wins / ties = the number of (positive p, negative q) with
 *              s_p > s_q / s_p == s_q.  Exact integers: AUC = (wins + ties / 2) / (n_pos n_neg) is the host's division
 *   ap_out     fp64 [n_out] = (1 / n_pos) sum_p pos_ge(p) / all_ge(p), pos_ge / all_ge = the positives / all pairs with
 *              score >= s_p (average precision, ties grouped: sklearn's definition).  fp64 quotients; the positives of a
 *              CSR row are added in entry order (first occurrences), then the rows' sums first row to last
 *   loss_out   fp32 [n_out] = gae_decoder_bce_graphs's l_g without dropout (train_inductive.py:44-48 on this graph
 *              alone): all n^2 ordered pairs, self pairs included, y_ij = the number of entries j in row i,
 *              pos_weight = (n^2 - S) / S; fp32 terms, fp64 sums per row, rows added first to last
 * DEGENERATE SLOTS: n_pos = 0: loss NaN; n_pos = 0 or n_neg = 0: ap NaN (wins = ties = 0; an empty graph gives zeros).
 * A graph id outside [0, n_graphs), a node range outside [0, n_nodes], a graph of more than max_graph_nodes (<= 64)
 * rows, or a non-finite logit anywhere in the graph: the four counts -1, ap and loss NaN.  Row pointers and column ids
 * as gae_embed_graphs: nothing outside the arrays is read or written.
 * INDEPENDENCE: a graph's outputs are functions of that graph's rows alone, with the same bits in any subset, order,
 * position, repeat or run.  No float atomics.
 * SHAPES TAKEN: 0 <= n_layers <= 4, f_in and every width in 1..64, max_graph_nodes <= 64: gae_score_graphs_usable
 * (1 = taken; agrees with gae_embed_graphs_usable for n_layers >= 1).  Argument errors as gae_embed_graphs, plus
 * exclude_self outside {0, 1} (GAE_E_RANGE) and n_layers = 0 with uint8 rows (GAE_E_DTYPE).  One launch, no workspace. */
int gae_score_graphs_usable(int64_t f_in, int64_t n_layers, const int64_t *widths, int64_t max_graph_nodes);

int gae_score_graphs(const int64_t *graph_ptr, int64_t n_graphs, int64_t n_nodes, int64_t n_edges,
                     int64_t max_graph_nodes, const int32_t *indptr, const int32_t *indices,
                     const void *feat, int feat_dtype, int64_t ldf, int64_t f_in, int64_t n_layers,
                     const int64_t *widths, const float *const *weights, const int64_t *ldw,
                     const float *const *biases, const int *acts, int norm, const int64_t *graph_ids,
                     int64_t n_out, int exclude_self, int64_t *counts_out, double *ap_out, float *loss_out,
                     void *stream);

/* ---- K23: k-means over the rows of an embedding, on the device (ops.kmeans, ops.kmeans_assign, GAE.cluster_nodes)
 * Node clustering, the second downstream task of a graph auto-encoder: Lloyd iterations and k-means++ seeding without
 * the n x k distance matrix, without float atomics and without a host round trip per iteration.
 *   X            fp32 [n, d], rows ldx >= d floats apart (any ldx: no alignment is asked for)
 *   C            fp32 [k, d], dense
 *   1 <= d <= 64, 1 <= k <= 256 (else GAE_E_RANGE); 0 <= n < 2^31, k <= n (else GAE_E_SIZE).  No fallback for other shapes.
 *   workspace    device memory of at least the workspace query's bytes: a pure host function of (n, d, k), positive,
 *                non-decreasing in n; a negative error code for the argument errors above.  A step keeps nothing in it
 *                between calls; the seeding and the steps may share one.
 * ASSIGNMENT (gae_kmeans_assign; the first launch of a step): row i goes to argmin_c |x_i - c_c|^2, evaluated in fp32 as
 * h_c - x_i . c_c with h_c = |c_c|^2 / 2 (an ascending-f fmaf chain, halved), the products on v_mfma_f32_32x32x2_f32 in the
 * fixed feature order of csrc/decoder_pairs.h.  Ties -- equal computed fp32 values, duplicate centres -- go to the LOWER
 * centre index.  dist2 of the chosen centre a is taken directly: the fmaf chain over f = 0 .. d - 1 ascending, from 0.f,
 * of (x_if - c_af)^2 -- no cancellation of the expanded form.  labels_out int32 [n]; dist2_out fp32 [n] or NULL.
 * STEP (gae_kmeans_step): one Lloyd iteration in four launches -- assign (labels in/out: the rows whose label differs
 * from the one found on entry are counted, -1 on entry counts as changed), cluster sums, fold, finish:
 *   sums         blocks own fixed contiguous row ranges, every accumulator has one writer that adds its rows in
 *                ascending order, the block partials are added in the library's one order for partial lists (common.h
 *                sum_partials), counts as int64.  The grid is a function of n alone.  The same bits run to run and for
 *                any ldx; no float atomics
 *   update       new centre = sum / count (fp32), written to C in place; a cluster without rows KEEPS its centre
 *   status       a 48-byte device block, zeroed by the caller before the first step:
 *                  done        set by the step when changed == 0 or shift2 <= tol_abs
 *                  iterations  += 1 per step that ran
 *                  changed     labels that differ from the ones on entry
 *                  empty       clusters without rows in this step
 *                  inertia     sum_i dist2_i of the labels against the centres they were chosen with (the C on entry):
 *                              fp64; per block of rows thread t adds rows t, t + 256, ... then a halving tree, the blocks
 *                              in sum_partials' 64-lane order
 *                  shift2      sum_c |c_new - c_old|^2: fp64, per centre in ascending f, the centres in ascending c
 *                Every kernel of a LATER step on a status whose done is set returns at once and touches neither C nor
 *                labels nor status: iterations may be enqueued in groups and the block read once per group, and the
 *                result has the same bits whatever the group size.
 *   tol_abs      double; negative: stop on changed == 0 only; NaN is GAE_E_RANGE.  flags: 0 (other bits GAE_E_RANGE)
 * SEEDING (gae_kmeans_init_pp): k-means++ as an exponential race, all k rounds enqueued by one call, one launch each.
 * key = seed ^ 0x9E3779B97F4A7C15.  Round 0 picks row philox4x32_10(ctr = 0, draw = 0, key)[0] mod n.  Round r >= 1:
 * mind2_i = min(mind2_i, |x_i - x_prev|^2) (direct, ascending-f fmaf chain), m_i = philox4x32_10(ctr = i, draw = r, key)[0]
 * >> 8, u_i = (m_i + 0.5) 2^-24, pick = argmax_i mind2_i / (-log u_i) in fp32 (-log u as -logf(u) for m_i < 2^23, else
 * -log1pf(-(2^24 - 1 - m_i + 0.5) 2^-24): both arguments exact), the LOWEST i among equal keys -- sampling with
 * probability proportional to D^2.  The pick does not depend on the grid.  chosen_out int32 [k]: the rows, distinct
 * unless X has fewer than k distinct rows (all keys 0: the lowest index wins; duplicate centres are legal input to a
 * step); C_out fp32 [k, d]: their rows, bit for bit.
 * Argument errors are returned before any launch: the shape errors above, ldx < d (GAE_E_SIZE), NULL X / C / labels /
 * status / outputs / workspace (GAE_E_NULL), a short workspace (GAE_E_WORKSPACE).  Non-finite X is the caller's
 * business (ops.kmeans checks): nothing outside the arrays is read or written, the labels stay inside [0, k). */
typedef struct gae_kmeans_status {
    int64_t done, iterations, changed, empty;
    double inertia, shift2;
} gae_kmeans_status;

int64_t gae_kmeans_workspace_bytes(int64_t n, int64_t d, int64_t k);

int gae_kmeans_assign(const float *X, int64_t ldx, int64_t n, int64_t d, const float *C, int64_t k,
                      int32_t *labels_out, float *dist2_out, void *workspace, int64_t workspace_bytes, void *stream);

int gae_kmeans_step(const float *X, int64_t ldx, int64_t n, int64_t d, float *C, int64_t k, int32_t *labels,
                    gae_kmeans_status *status, double tol_abs, int flags, void *workspace, int64_t workspace_bytes,
                    void *stream);

int gae_kmeans_init_pp(const float *X, int64_t ldx, int64_t n, int64_t d, int64_t k, uint64_t seed, float *C_out,
                       int32_t *chosen_out, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- K24: exact k-nearest-neighbour search over embeddings (ops.knn, GAE.nearest_nodes, GAE.nearest_graphs)
 * For every query row q_i of Q fp32 [m, d] (rows ldq floats apart) the k rows x_j of the database X fp32 [n, d] (ldx)
 * that are nearest to it, without the m x n matrix.  No alignment is asked of ldq / ldx / ldo.
 * METRICS  GAE_KNN_L2: squared Euclidean distance, smallest first.  GAE_KNN_DOT: inner product, largest first.  Cosine is
 *   not a kernel metric: the caller divides the rows by their norms and asks for GAE_KNN_DOT (ops.knn does).
 * CANDIDATES of query i: every database row j in [0, n) whose key (below) is neither NaN nor +-inf, minus j = i under
 *   GAE_KNN_EXCLUDE_SAME_INDEX (for Q = X: a row is not its own neighbour).
 * PRODUCTS  p_ij = q_i . x_j is the fp32 chain of csrc/decoder_pairs.h: v_mfma_f32_32x32x2_f32 (bitwise a k-ordered fmaf
 *   chain from 0.f) in K16's fixed feature order, the same lane width and chunk choice per d, chunks ascending.  With
 *   Q = X = Z it has the bits of gae_decoder_topk's s_ij.  It does not depend on tile position, split or schedule.
 * SELECTION KEY  DOT: key = p_ij.  L2: key = p_ij - h_j, h_j = (fmaf chain of x_jf^2, f ascending from 0.f) / 2, computed
 *   once per call into the workspace by a small first launch (|q - x|^2 / 2 = |q|^2 / 2 - key: the same order for one
 *   query).  The k candidates with the LARGEST key are chosen; equal keys go to the lower j.
 * REPORTED VALUE  DOT: the key.  L2: sum_f (q_if - x_jf)^2 taken directly -- an fmaf chain in ascending f from 0.f, as
 *   gae_kmeans_assign's dist2: no cancellation of the expanded form reaches the output.
 * ORDER OF A ROW  DOT: (value descending, j ascending).  L2: (reported value ascending, j ascending): the k chosen
 *   entries are re-sorted by the direct distance, so the distances of a row are monotone.  Fewer than k candidates pad
 *   the row's tail with index -1 and value +inf (L2) or -inf (DOT).
 * DETERMINISM  No float atomics, ordinary launches only.  The result is a function of the values of Q and X and of
 *   (m, n, d, k, metric, flags) alone: the same bits run to run, for any ldq / ldx / ldo and any `splits`.
 *   index_out    int32 [m, ldo >= k]: database rows;  value_out fp32 [m, ldo >= k]
 *   splits       column splits per group of query panels: 0 = auto, else 1 .. 16.  An argument, not a tuning knob
 *   workspace    device memory of at least gae_knn_workspace_bytes(m, n, d, k, splits) bytes: a pure host function,
 *                positive, non-decreasing in m, n, k and splits (1 .. 16); a negative error code for a shape error.
 *                O(n + m k splits) bytes, never O(m n)
 *   stream       a hipStream_t, passed as void * like everywhere in this library
 * 1 <= d <= 256, 1 <= k <= 64 (else GAE_E_RANGE); 0 <= m, n < 2^31 (else GAE_E_SIZE).  m = 0 and n = 0 are valid: with
 * n = 0 every row is padding.  There is no fallback for other shapes.
 * Argument errors are returned before anything is dereferenced or launched (no GPU is needed to see them): the shape
 * errors above, splits outside 0..16, an unknown metric or flag bit (GAE_E_RANGE), ldq < d, ldx < d, ldo < k
 * (GAE_E_SIZE), NULL index_out / value_out / Q (m > 0), NULL X (m, n > 0), NULL workspace (GAE_E_NULL), a short
 * workspace (GAE_E_WORKSPACE).
 * Launches: h (L2), the sweep, the merge of the splits' lists (splits > 1), the direct distances and re-sort (L2). */
enum { GAE_KNN_L2 = 0, GAE_KNN_DOT = 1 };
enum { GAE_KNN_EXCLUDE_SAME_INDEX = 1 };

int64_t gae_knn_workspace_bytes(int64_t m, int64_t n, int64_t d, int64_t k, int splits);

int gae_knn(const float *Q, int64_t ldq, int64_t m, const float *X, int64_t ldx, int64_t n, int64_t d, int64_t k,
            int metric, int flags, int splits, int32_t *index_out, float *value_out, int64_t ldo,
            void *workspace, int64_t workspace_bytes, void *stream);

/* ---- K25: ridge regression on a frozen feature with a k-fold CV lambda path (ops.ridge, GAE.ridge_graphs)
 * The first row of the reference's chemistry table ("GAE + Ridge" on the [mean | sum | max] molecule feature): closed
 * form, deterministic, lambda chosen by cross-validation from ONE pass over X -- every fold's fit and every fold's
 * held-out error follow from per-fold second moments.
 *   X            fp32 [n, d], rows ldx >= d floats apart;  Y fp32 [n, t], rows ldy >= t apart (no alignment asked)
 *   pivot        fp32 [d + t] (p_x, then p_y) or NULL = zeros.  v_i = [1, x_i - p_x, y_i - p_y], width W = 1 + d + t; the
 *                subtraction is done in fp64 after widening (exact for fp32 values of comparable exponent).  The fitted
 *                model does not depend on the pivot mathematically; a pivot near the column means keeps the moments small
 *   1 <= d <= 128, 1 <= t <= 8, 1 <= folds <= 32, 1 <= n_lambdas <= 64 (else GAE_E_RANGE); 0 <= n, n_rows < 2^31 (else
 *   GAE_E_SIZE).  There is no fallback for other shapes.
 * MOMENTS (gae_ridge_stats): for every fold f, M_f = sum_{i in fold f} v_i v_i^T in fp64, as a packed upper triangle:
 *   stats[f][i W - i (i - 1) / 2 + (j - i)] = M_f[i][j], 0 <= i <= j < W (fp64 [folds][W (W + 1) / 2]).
 *   rows         int32 [n_rows]: row ids of X / Y, ascending inside each fold; fold f owns rows[fold_ptr[f] ..
 *                fold_ptr[f + 1]).  fold_ptr is DEVICE int32 [folds + 1], 0 <= fold_ptr[0] <= ... <= fold_ptr[folds] ==
 *                n_rows.  rows = NULL means rows 0 .. n - 1, all in fold 0 (then n_rows == n and folds == 1, fold_ptr is
 *                ignored).  Rows that are not listed are never read.
 *   products     on v_mfma_f64_16x16x4_f64, the upper-triangle tiles of M split over the waves of a block.
 *   determinism  each fold's list is cut into chunks of GAE_RIDGE_CHUNK_ROWS rows (a constant, not a function of the
 *                device); a chunk never straddles folds; one block per chunk adds its rows in ascending list order,
 *                four per product; the chunk partials go to the workspace and a second launch adds each fold's partials
 *                in ascending chunk order, in THE order of partial lists (csrc/common.h sum_partials, here in fp64: <= 32
 *                partials one lane in order; more: 64 lanes, lane l adds l, l + 64, ..., then the shuffle-down tree).
 *                No float atomics.  stats is a function of the listed values and the fold lists alone: the same bits
 *                run to run, for any ldx / ldy and any stream.  A fold without rows gives an all-zero block.
 *   status       a 32-byte device block the caller zeroes; the launches only add to it:
 *                  nonfinite_rows  listed rows that hold a NaN or an infinity in X or Y (integer atomics)
 *                  errors          GAE_RIDGE_ERR_FOLD_PTR: fold_ptr is not monotone from >= 0 to n_rows -- nothing is read
 *                                  through it and stats is filled with NaN;  GAE_RIDGE_ERR_ROW_ID: a row id outside [0, n)
 *                                  -- the row is skipped;  GAE_RIDGE_ERR_LAMBDA (gae_ridge_solve): a lambda that is
 *                                  negative or not finite
 *   workspace    device memory of at least gae_ridge_workspace_bytes(n_rows, d, t, folds) bytes: a pure host function,
 *                positive, non-decreasing in n_rows; a negative error code for a shape error.
 * MODELS (gae_ridge_solve): one launch, one block per (model m in 0 .. folds, lambda index l).  Model m < folds trains on
 * every fold but m, model `folds` on all listed rows.
 *   1. S = sum of M_f over the training folds, f ascending;  c = S[0][0], mu = S[0][1:] / c;  C = S[1:, 1:] - c mu mu^T
 *   2. A = C_xx + lambda I: the intercept is not penalised.  GAE_RIDGE_NO_INTERCEPT: no centring; the moments are moved
 *      back from the pivot to the origin first, so the model is y = x^T w for any pivot
 *   3. fp64 Cholesky of the packed triangle in LDS;  4. forward and back substitution for the t right-hand sides
 *   5. intercept b = p_y + mu_y - mu_x^T w - p_x^T w
 *   The held-out squared error of fold m comes from the moments too: with b' = b - p_y + p_x^T w and u = [-b', -w, e_j],
 *   cv_sse[m][l][j] = u^T M_m u.  X is not read again.
 *   coef fp64 [folds + 1][L][t][d];  intercept fp64 [folds + 1][L][t];  cv_sse fp64 [folds][L][t];
 *   info int32 [folds + 1][L], LAPACK style: 0, or the 1-based index of the first pivot that is <= 0 or not finite; -1:
 *   the model's training set is empty (c = 0); -2: its lambda is negative or not finite.  Where info != 0 the cell's
 *   coefficients, intercept and SSE are NaN.  lambdas: DEVICE fp64 [L].  pivot: the one the moments were taken with.
 * Argument errors are returned before anything is dereferenced or launched (no GPU is needed to see them): the shape
 * errors above, ldx < d, ldy < t, rows = NULL with n_rows != n or folds != 1 (GAE_E_SIZE), unknown flag bits (GAE_E_RANGE),
 * NULL X / Y (n_rows > 0), fold_ptr (rows given), stats, status, workspace, lambdas or an output (GAE_E_NULL), a short
 * workspace (GAE_E_WORKSPACE). */
enum { GAE_RIDGE_CHUNK_ROWS = 256 };
enum { GAE_RIDGE_NO_INTERCEPT = 1 };
enum { GAE_RIDGE_ERR_FOLD_PTR = 1, GAE_RIDGE_ERR_ROW_ID = 2, GAE_RIDGE_ERR_LAMBDA = 4 };

typedef struct gae_ridge_status {
    int64_t nonfinite_rows, errors, reserved[2];
} gae_ridge_status;

int64_t gae_ridge_workspace_bytes(int64_t n_rows, int64_t d, int64_t t, int64_t folds);

int gae_ridge_stats(const float *X, int64_t ldx, const float *Y, int64_t ldy, int64_t n, int64_t d, int64_t t,
                    const float *pivot, const int32_t *rows, int64_t n_rows, const int32_t *fold_ptr, int64_t folds,
                    double *stats, gae_ridge_status *status, void *workspace, int64_t workspace_bytes, void *stream);

int gae_ridge_solve(const double *stats, int64_t d, int64_t t, int64_t folds, const float *pivot, const double *lambdas,
                    int64_t n_lambdas, int flags, double *coef, double *intercept, double *cv_sse, int32_t *info,
                    gae_ridge_status *status, void *stream);

/* ---- K26: a histogram-based regression forest on a frozen feature (ops.forest, GAE.forest_graphs, embed --forest)
 * The third row of the reference's chemistry table ("GAE + Random Forest").  EVERY ACCUMULATED QUANTITY IS AN INTEGER:
 * features become bin codes, targets fixed-point int64, histogram cells integer counts and integer sums.  Integer atomics
 * in LDS and in global memory are exact and free of order: no float atomics, the same bits run to run, for any row
 * stride, stream or launch split, and a numpy restatement (tests/forest_ref.py) reproduces every tree node for node.
 * Regression only; gradient boosting (with binary classification) is K30.
 *   1 <= d <= 256, 1 <= t <= 8, 1 <= n_trees <= 1024, 1 <= max_depth <= 16, 2 <= max_bins <= 256 (else GAE_E_RANGE);
 *   1 <= n_used, n_boot < 2^31, 0 <= n, m < 2^31 (else GAE_E_SIZE).  There is no fallback for other shapes.
 * BINNING (gae_forest_bin): per feature f an ascending fp32 edge list edges[f][0 .. n_edges[f]), n_edges[f] <= max_bins - 1
 *   (edges: DEVICE fp32 [d][max_bins - 1], entries past n_edges[f] are not read; n_edges: DEVICE int32 [d]).
 *   code(x) = #{e in edges[f] : e < x}, a uint8: a binary search over the edge lists held in LDS.  codes_out is uint8
 *   [n_rows][d], row-major by LISTED row: row i of it belongs to X's row rows[i] (rows = NULL: rows 0 .. n - 1, then
 *   n_rows == n).  The histogram launch gathers d contiguous bytes per sample from it.  Rows that are not listed are
 *   never read.  A feature without edges is constant and can never split.  ops.forest computes the edges with torch
 *   from a column sort of the listed rows: at most max_bins distinct values -> the midpoints of consecutive distinct
 *   values a < b, (double(a) + double(b)) / 2 rounded to fp32, and a itself where that rounds up to b, so a <= edge < b
 *   and the binning is lossless; more -> the order statistics v[(k n_used) / max_bins], k = 1 .. max_bins - 1 (integer
 *   division) of the sorted column v, de-duplicated.  An edge of -0 is stored as +0 (they compare equal).
 * TARGETS: Y fp32 [n][t] (ldy).  Per target j a pivot c_j (fp32) and an integer exponent e_j, HOST arrays of t values;
 *   the device forms y_q = rint((double(y) - double(c_j)) 2^e_j) as int64 (ties to even).  ops.forest takes c_j = the fp64
 *   mean of the listed rows rounded to fp32 and e_j = 30 - E_j with frexp(max_i |double(y_ij) - double(c_j)|) = (m, E_j),
 *   0.5 <= m < 1 (e_j = 0 when that max is 0): |y_q| <= 2^30, a sum over up to 2^31 samples fits an int64, and the
 *   quantisation step is 2^-31 of the target's range.  -200 <= e_j <= 200.
 * BOOTSTRAP (GAE_FOREST_BOOTSTRAP): tree T trains on n_boot samples; sample j is listed row (w n_used) >> 32 (64-bit
 *   product) with w = word j & 3 of philox4x32_10(ctr = j >> 2, draw = T, key = seed ^ GAE_FOREST_KEY_XOR) (csrc/common.h).
 *   Without the flag sample j is listed row j and n_boot == n_used.  inbag (uint8 [n_trees][n_used] or NULL) is zeroed
 *   and then holds 1 where tree T drew listed row i (integer stores).
 * GROWTH, level by level, all trees at once.  The root is node 0.  A node at depth < max_depth with count >= 2
 *   min_samples_leaf is offered a split.  Candidate (f, b), 0 <= b < n_edges[f], sends a sample left iff code_f <= b; both
 *   children need count >= min_samples_leaf.  With S_Lj, S_Rj the children's exact integer sums of y_q for target j:
 *     score = sum_j ((double(S_Lj) double(S_Lj)) / double(n_L) + (double(S_Rj) double(S_Rj)) / double(n_R)) 4^(-e_j)
 *   in fp64: convert, square, divide, add the two sides, scale, then add over j ascending from 0.0 -- without contraction
 *   (csrc/forest.hip is built with -ffp-contract=off).  The parent's score is sum_j ((double(S_j) double(S_j)) /
 *   double(n)) 4^(-e_j), computed the same way.  The best candidate has the largest score; ties go to the lower f, then
 *   the lower b.  The node splits iff best > parent (strictly); gain = best - parent.  So a pure node is a leaf.
 *   max_features = m < d: the candidates of node v of tree T are the m features with the smallest (r_f, f), r_f = word 0
 *   of philox4x32_10(ctr = (v << 8) | f, draw = 2^32 + T, key).
 * NODE NUMBERING: with `base` the tree's node count before a level is split, the k-th splitting node of the level in
 *   ascending id (k from 0) gets the children base + 2 k (left) and base + 2 k + 1: independent of scheduling.
 * NODE TABLES, [n_trees][node_capacity], node_capacity == min(2^(max_depth + 1) - 1, 2 n_boot - 1):
 *   feature int32 (-1: a leaf), threshold_bin int32 (b; -1), threshold fp32 (edges[f][b]; 0), left int32 (the right child
 *   is left + 1; -1), count int32, value fp64 [..][t] = double(c_j) + (double(S_j) / double(count)) 2^(-e_j) for EVERY
 *   node, gain fp64 (0 for a leaf); n_nodes int32 [n_trees].  Slots past n_nodes hold the leaf defaults with count 0 and
 *   value 0: gae_forest_fit writes every slot.
 * HOT PATH: each tree's sample list stays partitioned by node; a block owns (node chunk, feature tile), builds the
 *   tile's cells in LDS with integer atomics, scans the bins and emits the tile's best candidate only.  A node longer
 *   than GAE_FOREST_SPLIT_ROWS samples is cut across blocks whose cells are merged by integer atomics before the scan:
 *   the result cannot depend on the cut.  The host reads one 32-byte level status per level (gae_forest_fit
 *   synchronises the stream max_depth - 1 times at most).
 * PREDICTION (gae_forest_predict): X fp32 [m][d] (ldx).  Each row walks every tree on the raw floats, left iff x_f <=
 *   threshold -- the partition code_f <= b of the fit, a value exactly on an edge included.  out fp64 [m][t] = (sum of
 *   the reached nodes' values, trees ascending) / (trees added).  skip (uint8 [n_trees][m] or NULL): a non-zero entry
 *   omits the tree for the row (inbag of the fit gives the out-of-bag prediction); a row every tree skips gets NaN.  A
 *   row holding a non-finite feature is counted in status.nonfinite and gets NaN.  A walk that leaves the table (child
 *   ids outside 1 .. node_capacity - 1, feature >= d, more than 64 steps) stops: GAE_FOREST_ERR_NODE, NaN for the row.
 * STATUS: a 32-byte device block the caller zeroes; launches only add to it.  nonfinite: non-finite values of listed rows
 *   (gae_forest_bin: X; gae_forest_fit: Y), rows (gae_forest_predict).  errors: GAE_FOREST_ERR_ROW_ID a row id outside
 *   [0, n) (skipped), GAE_FOREST_ERR_NODE a broken node table, GAE_FOREST_ERR_CODE a code >= max_bins (skipped).
 * workspace: device memory of gae_forest_workspace_bytes(...) bytes at least: a pure host function, positive; a negative
 *   error code for a shape error.  Argument errors are returned before anything is dereferenced or launched (no GPU is
 *   needed to see them): the shape errors above, max_features outside 1 .. d, min_samples_leaf < 1, unknown flags
 *   (GAE_E_RANGE), ldx < d, ldy < t, rows = NULL with n_rows != n, n_boot != n_used without the bootstrap, another
 *   node_capacity (GAE_E_SIZE), a NULL array (GAE_E_NULL), a short workspace (GAE_E_WORKSPACE). */
enum { GAE_FOREST_SPLIT_ROWS = 8192 };
enum { GAE_FOREST_BOOTSTRAP = 1 };
enum { GAE_FOREST_ERR_ROW_ID = 1, GAE_FOREST_ERR_NODE = 2, GAE_FOREST_ERR_CODE = 4 };
#define GAE_FOREST_KEY_XOR 0xA0761D6478BD642FULL

typedef struct gae_forest_status {
    int64_t nonfinite, errors, reserved[2];
} gae_forest_status;

int64_t gae_forest_workspace_bytes(int64_t n_used, int64_t d, int64_t t, int64_t n_trees, int64_t n_boot, int64_t max_depth,
                                   int64_t max_bins);

int gae_forest_bin(const float *X, int64_t ldx, int64_t n, int64_t d, const int32_t *rows, int64_t n_rows,
                   const float *edges, const int32_t *n_edges, int64_t max_bins, uint8_t *codes_out,
                   gae_forest_status *status, void *stream);

int gae_forest_fit(const uint8_t *codes, const int32_t *n_edges, const float *edges, int64_t n_used, int64_t d,
                   int64_t max_bins, const float *Y, int64_t ldy, int64_t n, int64_t t, const int32_t *rows,
                   const float *pivot, const int32_t *exponent, int64_t n_trees, int64_t n_boot, int64_t max_depth,
                   int64_t max_features, int64_t min_samples_leaf, int flags, uint64_t seed, int32_t *feature,
                   int32_t *threshold_bin, float *threshold, int32_t *left, int32_t *count, double *value, double *gain,
                   int32_t *n_nodes, int64_t node_capacity, uint8_t *inbag, gae_forest_status *status, void *workspace,
                   int64_t workspace_bytes, void *stream);

int gae_forest_predict(const float *X, int64_t ldx, int64_t m, int64_t d, int64_t t, int64_t n_trees, int64_t node_capacity,
                       const int32_t *feature, const float *threshold, const int32_t *left, const double *value,
                       const uint8_t *skip, double *out, gae_forest_status *status, void *stream);

/* ---- K30: second-order histogram gradient boosting on a frozen feature (ops.boost, GAE.boost_graphs, embed --boost)
 * XGBoost's objective on integer histograms, for regression ("squared") and binary classification ("logistic").  EVERY
 * ACCUMULATED QUANTITY IS AN INTEGER and every floating-point step is a stated fp64 operation without contraction
 * (csrc/boost.hip is built with -ffp-contract=off), so tests/boost_ref.py restates a whole fit bit for bit, and the
 * results do not depend on the run, the stream, check_every or on which other configurations share the call.
 *   1 <= d <= 256, 2 <= max_bins <= 256, 1 <= max_depth <= 8, 1 <= n_rounds <= 4096, folds = 0 or 2..255,
 *   (folds + 1) n_cfg <= 256 models, 0 < learning_rates[c] <= 1, lambdas[c] >= 0, min_child_weight > 0 or every lambda > 0
 *   (else GAE_E_RANGE); 1 <= n_used < 2^31 (else GAE_E_SIZE).  One target, binary labels.  There is no fallback.
 * INPUTS, all by LISTED row: codes uint8 [n_used][d] with edges / n_edges as gae_forest_bin made them (K26 BINNING); y fp32
 *   [n_used] (logistic: exactly 0 or 1, else GAE_BOOST_ERR_TARGET; squared: finite, else the same flag); fold int32 [n_used]
 *   in 0 .. folds - 1 (else GAE_BOOST_ERR_FOLD; NULL with folds = 0).  learning_rates, lambdas: HOST fp64 [n_cfg], one pair
 *   per configuration.
 * MODELS: m = cfg (folds + 1) + k; k < folds trains on the rows with fold != k and is scored on the rows with fold == k,
 *   k == folds trains on every row.  All models start from F = base_score and run side by side in the same launches.
 * FRAME: g and h become int64 fixed point, q = llrint(v 2^e) (ties to even).  logistic: e = 30 for both.  squared: h is the
 *   integer 1 and g uses the caller's exponent; ops.boost takes base_score = the fp32-rounded fp64 mean of y and e = 29 - E
 *   with frexp(max |y - base_score|) = (m, E) (e = 0 when that max is 0), so |g 2^e| stays below 2^31 while |F - y| is at
 *   most twice that max, and a sum over 2^31 rows fits an int64.  A value with |v 2^e| > 2^31 (or a non-finite F) sets
 *   bad[m] = 1 and contributes 0: nothing wraps.  G = double(sum q_g) 2^-e and H = double(sum q_h) 2^-e_h below.
 * SIGMA, no libm: a = min(|F|, 40) (a NaN takes 40); k = rint(-a 1.44269504088896338700e+00); r = (-a - k
 *   6.93147180369123816490e-01) - k 1.90821492927058770002e-10; P = the Horner form p = 1/13!, p = p r + 1/j! for j = 12 .. 0
 *   (coefficients the correctly rounded quotients); e = P 2^k (exact scaling); q = e / (1 + e); sigma = F >= 0 ? 1 - q : q.
 *   p = sigma(F), g = p - y, h = p (1 - p).  squared: g = F - double(y).
 * ROUND r = 0 .. n_rounds - 1.  Prologue, per (model, listed row): F += value[leaf of the model's tree of round r - 1 on
 *   the row's codes] (r > 0; code_f <= threshold_bin goes left), then g, h, q as above; the model's training rows and their
 *   integer sums make the root.  Held-out rows add their loss -- squared (F - y)^2; logistic log1p(e) + (|F| when the sign of
 *   F disagrees with y), e as in SIGMA (libm's log1p: it feeds the selection, never a tree) -- per chunk of 256 listed rows:
 *   within a wave the shuffle-down tree 32, 16, .., 1, then ((w0 + w1) + w2) + w3; the chunks are folded in the order of
 *   csrc/common.h's sum_partials (<= 32 chunks: ascending; more: 64 strided lanes ascending, then the same tree) into
 *   loss[m][r].  correct[m][r] counts held-out rows with (F >= 0) == (y == 1) (logistic; 0 for squared).  So loss[m][r] is the
 *   model's held-out loss SUM with r trees; a last prologue after the last round fills index n_rounds and leaves the final F
 *   in score.  There are no float atomics.
 * GROWTH as K26's, level by level: the root is node 0; a node at depth < max_depth with count >= 2 min_samples_leaf is
 *   offered a split.  Candidate (f, b), 0 <= b < n_edges[f], needs n_L, n_R >= min_samples_leaf, H_L, H_R >= min_child_weight
 *   and H_L + lambda, H_R + lambda > 0; score = (G_L G_L) / (H_L + lambda) + (G_R G_R) / (H_R + lambda), the right side from
 *   the integer differences to the node's sums.  The largest score wins, ties to the lower f, then the lower b.  The node
 *   splits iff best > parent + min_gain with parent = (G G) / (H + lambda) (0 when H + lambda is not > 0); gain = best -
 *   parent.  value = -(lr (G / (H + lambda))) for EVERY node (0 when H + lambda is not > 0): the leaf weight with the
 *   learning rate applied.  max_features = m < d: K26's subset rule with draw = 2^32 + ((r << 8) | k) -- the model's fold
 *   slot k, not its configuration, so a configuration gives the same trees alone or inside a grid.  NODE NUMBERING as K26.
 * OUTPUTS: the all-rows models' node tables [n_cfg][n_rounds][node_capacity], node_capacity = 2^(max_depth + 1) - 1, with
 *   K26's fields and defaults (value fp64 [..] one per node); n_nodes int32 [n_cfg][n_rounds]; loss fp64 and correct int64
 *   [models][n_rounds + 1]; score fp64 [models][n_used]; bad int32 [models].  The fold models' trees live in per-round scratch.
 * HOT PATH: the level kernels of K26 with (count, G, H) cells; each model owns fixed regions of the work lists and a 16-byte
 *   level record that stays on the device; every grid is sized by its bound -- level l has at most 2^l nodes and 2^l +
 *   ceil(n_used / GAE_FOREST_SPLIT_ROWS) chunks per model -- and surplus blocks return at once.  3 + 4 max_depth launches per
 *   round at most.  The host reads the status block once per check_every rounds (and stops early only when it already holds an
 *   error or every model is bad) -- no result depends on check_every.
 * PREDICTION (gae_boost_predict): tables of ONE configuration [n_rounds][node_capacity]; out fp64 [m] = base_score + the
 *   reached leaves' values added in ascending round order; a row goes left iff x_f <= threshold.  A row holding a non-finite
 *   feature is counted in status.nonfinite and gets NaN; a walk that leaves the table: GAE_FOREST_ERR_NODE, NaN.
 * STATUS: gae_forest_status, zeroed by the caller; errors holds GAE_FOREST_ERR_* and GAE_BOOST_ERR_* bits, reserved[0] the
 *   number of models marked bad.  Argument errors are returned before anything is dereferenced or launched. */
enum { GAE_BOOST_SQUARED = 0, GAE_BOOST_LOGISTIC = 1 };
enum { GAE_BOOST_ERR_TARGET = 8, GAE_BOOST_ERR_FOLD = 16 };

int64_t gae_boost_workspace_bytes(int64_t n_used, int64_t d, int64_t max_bins, int64_t max_depth, int64_t folds, int64_t n_cfg);

int gae_boost_fit(const uint8_t *codes, const int32_t *n_edges, const float *edges, int64_t n_used, int64_t d, int64_t max_bins,
                  const float *y, const int32_t *fold, int64_t folds, int objective, double base_score, int32_t exponent,
                  const double *learning_rates, const double *lambdas, int64_t n_cfg, int64_t n_rounds, int64_t max_depth,
                  int64_t max_features, int64_t min_samples_leaf, double min_child_weight, double min_gain, uint64_t seed,
                  int64_t check_every, int32_t *feature, int32_t *threshold_bin, float *threshold, int32_t *left, int32_t *count,
                  double *value, double *gain, int32_t *n_nodes, double *loss, int64_t *correct, double *score, int32_t *bad,
                  gae_forest_status *status, void *workspace, int64_t workspace_bytes, void *stream);

int gae_boost_predict(const float *X, int64_t ldx, int64_t m, int64_t d, int64_t n_rounds, int64_t node_capacity,
                      const int32_t *feature, const float *threshold, const int32_t *left, const double *value,
                      double base_score, double *out, gae_forest_status *status, void *stream);

/* ---- K27: a small MLP regression head trained on a frozen feature (ops.mlp, GAE.mlp_graphs, embed --mlp)
 * The best row of the reference's chemistry table ("GAE + MLP").  d -> h1 [-> h2] -> t (h2 = 0: one hidden layer), ReLU
 * on the hidden layers, identity on the output, squared error; regression only.  ONE block of 256 threads per model, all
 * models of a call in one grid; no grid-wide synchronisation and no atomics on floats; csrc/mlp.hip is built with
 * -ffp-contract=off.  The result is a function of the listed values and the arguments alone: the same bits run to run,
 * for any ldx / ldy, any number of models in the call and any cut into launches; tests/mlp_ref.py restates it in numpy.
 *   1 <= d, h1 <= 128, 0 <= h2 <= 128, 1 <= t <= 8, 1 <= n_models <= 4096, 1 <= n_lists <= 1024, batch_size >= 1 (else
 *   GAE_E_RANGE).  A shape inside these limits whose on-chip state passes a block's 160 KB of LDS (128 -> 128 -> 128 -> t)
 *   is GAE_E_RANGE from every entry point, gae_mlp_workspace_bytes included.  There is no fallback.
 * DATA: X fp32 [n, d] (ldx), Y fp32 [n, t] (ldy).  shift / scale: fp32 [d + t] each (features, then targets) or NULL (0 and
 *   1).  The model sees v' = (v - shift) * scale: a subtraction, then a multiplication, in fp32.
 *   rows int32 [n_rows]: lists of row ids, one after another; list k is rows[list_ptr[k] .. list_ptr[k + 1]) (list_ptr:
 *   DEVICE int32 [n_lists + 1], each pair 0 <= lo <= hi <= n_rows; lists may overlap).  Model m trains on list train_list[m]
 *   and is scored on list eval_list[m] (-1: none); lr, alpha fp32 [n_models], seed uint64 [n_models]: all DEVICE arrays.
 *   Rows in no list that a model of the call uses are never read.
 * LAYERS l = 0 .. L - 1 (L = 2 or 3) with W_l fp32 [out_l][in_l] (torch.nn.Linear layout) and b_l [out_l]:
 *   z_l = chain_k(a_l[k], W_l[j][k]) + b_l[j];  a_{l+1} = relu(z_l) = (z_l > 0 ? z_l : +0) for l < L - 1;  yhat = z_{L-1}.
 * ARITHMETIC.  chain_k(p_k, q_k) is ONE fp32 fma chain from +0 over the summed index in ascending order,
 *   c <- fma(p_k, q_k, c): the fp32-input matrix instruction (v_mfma_f32_16x16x4_f32) computes exactly that.  One chain
 *   per output element; waves split output tiles, never the summed index.  Operands past a matrix's edge are zeros.
 *     forward      summed over the in_l features / hidden units;
 *     output error delta_{L-1}[r][j] = yhat[r][j] - y'[r][j];
 *     dW_l[j][k]   = chain over the batch's rows r in batch order of (delta_l[r][j], a_l[r][k]): the batch is walked in
 *                  panels of 32 rows, the accumulators stay in registers across panels, so the chain continues;
 *     db_l[j]      = chain over the same rows of (delta_l[r][j], 1), that is c <- c + delta_l[r][j];
 *     delta_{l-1}[r][k] = (a_l[r][k] > 0) ? chain over j ascending of (delta_l[r][j], W_l[j][k]) : +0.
 *   Everything else is a single correctly rounded fp32 operation, in this order (B = the batch's own size as fp32):
 *     g = ((chain + alpha * w) / B) for a weight, g = chain / B for a bias (alpha * w = +0 there);
 *     GAE_MLP_ADAM: m = beta1 * m + (1 - beta1) * g;  v = beta2 * v + ((1 - beta2) * (g * g));
 *                  w = w - step * (m / (sqrtf(v) / c2 + eps)), with step = fp32(double(lr) / (1 - beta1^s)) and c2 =
 *                  fp32(sqrt(1 - beta2^s)) taken in fp64 and rounded once; s counts the model's batches from 1; beta^s is a
 *                  double in the state block, advanced by one multiplication per batch (as K12 does); (1 - beta) is fp32.
 *     GAE_MLP_SGD:  vel = momentum * vel - lr * g;  w = w + vel (vel lives in the first moment's place).
 *   fp32 division and sqrtf are the correctly rounded forms.
 * INITIALISATION (a launch with e0 == 0): Glorot uniform as sklearn's MLPRegressor draws it for ReLU: bound_l =
 *   fp32(sqrt(6.0 / (in_l + out_l))) (fp64, rounded once); element e (row-major) of W_l takes word e & 3 of
 *   philox4x32_10(ctr = e >> 2, draw = 2 l, key = seed) (csrc/common.h), element e of b_l the same with draw = 2 l + 1;
 *   u = (word >> 8) * 2^-24;  value = ((2 * u) - 1) * bound_l.  The moments start at 0, s at 0, the beta powers at 1.
 * MINI-BATCH ORDER: epoch e visits list positions perm_e(0), perm_e(1), ...; batch b is positions [b B, min((b + 1) B,
 *   n_train)): the last batch is short, B > n_train is one batch.  Without GAE_MLP_SHUFFLE perm_e(p) = p.  With it perm_e
 *   is a keyed bijection computed per position: let hb >= 1 be the smallest integer with 4^hb >= n_train, mask = 2^hb - 1;
 *   v = p; repeat { (hi, lo) = (v >> hb, v & mask); four rounds r = 0 .. 3: (hi, lo) <- (lo, hi ^ (F & mask)) with F = word
 *   0 of philox4x32_10(ctr = (r << 32) | lo, draw = 2^32 + e, key = seed); v = (hi << hb) | lo } until v < n_train.
 *   (draw >= 2^32: disjoint from the initialisation's streams.)
 * LOSS: loss_curve[m][e] (fp64 [n_models][epochs]) = (sum of double(delta)^2 on the scaled targets, added in fp64 in
 *   batch, row, target order) / (2 n_train).  After each epoch: if that value or any updated weight or bias of the epoch
 *   is not finite, info[m] = 1 + e, the model stops updating and the later entries of loss_curve are NaN.
 * EVALUATION (GAE_MLP_FINAL, after epoch e1 - 1): the rows of list eval_list[m] in list order, the same forward;
 *   err = ((yhat / scale_y) + shift_y) - y in fp32 (the targets' own units); eval_sse[m][j] (fp64 [n_models][t]) = the sum
 *   of double(err)^2 over the rows in that order.  NaN without an evaluation list or where info[m] != 0.
 * STATE: the workspace is n_models state blocks of S = gae_mlp_workspace_bytes(d, h1, h2, t, 1) bytes each (so the
 *   query is linear in n_models).  A block: int64 s; double beta1^s, beta2^s; int32 info, epochs done; 8 reserved floats
 *   (GAE_MLP_STATE_HEADER = 16 floats in all); then W_0, b_0, W_1, b_1 [, W_2, b_2] as fp32, P values; then the first
 *   moments in the same layout; then the second moments; zeros up to S (e0 == 0 writes the whole block).
 *   gae_mlp_fit runs epochs [e0, e1) of `epochs` from the block;
 *   e0 == 0 initialises it; e0 must equal the block's epochs done (else GAE_MLP_ERR_RESUME and info = -2).  ops.mlp cuts
 *   a fit into launches of at most GAE_MLP_LAUNCH_ROW_VISITS row visits per model (whole epochs, one at least), so a long
 *   fit is never one long-running kernel.  AN ESTIMATE until it is measured: about 1 us per row visit at the widest
 *   shape, a quarter of a second per launch.
 * info int32 [n_models]: 0; 1 + e as above; -1: the training list is empty or not a list; -2: a resume mismatch.
 * STATUS: a 32-byte device block the caller zeroes; launches only add to it (integer atomics).  nonfinite_rows: entries
 *   of the used lists whose row holds a NaN or an infinity in X or Y (counted by the e0 == 0 launch; a row in two lists
 *   counts twice), rows of gae_mlp_predict with a non-finite feature.  errors: GAE_MLP_ERR_LIST_PTR (a list_ptr pair outside
 *   0 <= lo <= hi <= n_rows: such a list is not read), GAE_MLP_ERR_ROW_ID (a row id outside [0, n): the row is taken as
 *   zeros), GAE_MLP_ERR_LIST_ID, GAE_MLP_ERR_RESUME.
 * PREDICTION (gae_mlp_predict): out fp32 [n_models][n][t] = (yhat / scale_y) + shift_y for every row of X and every state
 *   block of `state` (blocks S bytes apart, as the workspace holds them), with the forward chains of training.  A row
 *   holding a non-finite feature gives NaN and is counted (status may be NULL).
 * Argument errors are returned before anything is dereferenced or launched (no GPU is needed to see them): the limits
 *   above, an unknown solver or flag, betas or momentum outside [0, 1), eps <= 0, an epoch interval outside 0 <= e0 < e1 <=
 *   epochs (GAE_E_RANGE), n, n_rows outside int32, ldx < d, ldy < t (GAE_E_SIZE), a NULL array (GAE_E_NULL), a short
 *   workspace (GAE_E_WORKSPACE). */
enum { GAE_MLP_LAUNCH_ROW_VISITS = 262144 };
enum { GAE_MLP_STATE_HEADER = 16 };
enum { GAE_MLP_ADAM = 0, GAE_MLP_SGD = 1 };
enum { GAE_MLP_SHUFFLE = 1, GAE_MLP_FINAL = 2 };
enum { GAE_MLP_ERR_LIST_PTR = 1, GAE_MLP_ERR_ROW_ID = 2, GAE_MLP_ERR_LIST_ID = 4, GAE_MLP_ERR_RESUME = 8 };

typedef struct gae_mlp_status {
    int64_t nonfinite_rows, errors, reserved[2];
} gae_mlp_status;

int64_t gae_mlp_workspace_bytes(int64_t d, int64_t h1, int64_t h2, int64_t t, int64_t n_models);

int gae_mlp_fit(const float *X, int64_t ldx, const float *Y, int64_t ldy, int64_t n, int64_t d, int64_t h1, int64_t h2,
                int64_t t, const float *shift, const float *scale, const int32_t *rows, int64_t n_rows,
                const int32_t *list_ptr, int64_t n_lists, const int32_t *train_list, const int32_t *eval_list,
                const float *lr, const float *alpha, const uint64_t *seed, int64_t n_models, int64_t batch_size,
                float beta1, float beta2, float eps, int solver, float momentum, int flags, int64_t e0, int64_t e1,
                int64_t epochs, double *loss_curve, double *eval_sse, int32_t *info, gae_mlp_status *status,
                void *workspace, int64_t workspace_bytes, void *stream);

int gae_mlp_predict(const float *X, int64_t ldx, int64_t n, int64_t d, int64_t h1, int64_t h2, int64_t t,
                    const float *shift, const float *scale, const void *state, int64_t n_models, float *out,
                    gae_mlp_status *status, void *stream);

/* ---- K28: multinomial logistic regression on a frozen feature with a k-fold CV lambda path (ops.logreg,
 * GAE.classify_nodes, GAE.logreg_graphs, embed --logreg, train_transductive --classify)
 * The standard protocol for an unsupervised embedding: freeze it, fit a softmax classifier on the labelled rows, report
 * held-out accuracy.  Per model
 *   J(b, W) = sum_{i in training rows} -log softmax(b + W x~_i)[y_i] + (lambda / 2) sum_k |w_k|^2,   x~ = x - p
 * (sklearn's C = 1 / lambda; the intercepts are not penalised; p, the pivot, is fp32 [d] or NULL = zeros).
 *   X fp32 [n, d], rows ldx >= d floats apart;  y int32 [n] with the class of every LISTED row in 0 .. c - 1 (another value
 *   sets GAE_LOGREG_ERR_LABEL and the row enters without a label);  rows / fold_ptr: gae_ridge_stats' lists (rows int32
 *   [n_rows] ascending inside each fold, fold_ptr DEVICE int32 [folds + 1]).  Rows that are not listed are never read.
 *   1 <= d <= 128, 2 <= c <= 32, 1 <= folds <= 32, 1 <= n_lambdas <= 64, 1 <= model_batch <= models (else GAE_E_RANGE);
 *   0 <= n, n_rows < 2^31 (else GAE_E_SIZE).  There is no fallback for other shapes.
 * MODELS: models = (folds + 1) n_lambdas; model g = m n_lambdas + l trains at lambdas[l] on every fold but m (m < folds)
 * or on all listed rows (m = folds).  With D1 = d + 1 its parameters are [c][D1], column 0 the intercept about the pivot.
 * A caller may cut the models into launches [model_lo, model_lo + model_count), model_count <= model_batch; no model's
 * numbers depend on the cut or on the other models.
 * SOLVER: first order in the metric of a fixed majoriser, accelerated, with gradient restart.
 *   majoriser  S = sum [1, x~][1, x~]^T over the training rows; the Hessian is below S / 2 (x) I_c (Boehning), so
 *              A = S / 2 + lambda diag(0, 1 .. 1) is factorised ONCE per model and shared by the classes.  The step is
 *              invariant to an affine rescaling of the features.
 *   gae_logreg_factor: one block per model.  stats: gae_ridge_stats' output for t = 1 (width d + 2; the target's
 *              entries are ignored), taken with pivot [p, anything].  The training folds are added in ascending order, A
 *              is factorised by K25's fp64 Cholesky-Crout in LDS, the factor goes to the workspace.  The call also resets
 *              the state (W = W_prev = V = 0, t = 1) and the tables: info (LAPACK style as gae_ridge_solve: 0; j: pivot j
 *              <= 0 or not finite; -1: no training row; -2: lambda negative or not finite; later -3: the iteration left
 *              the finite numbers), n_iter = 0, converged = 0, coef / intercept 0 (NaN where info != 0);
 *              status.active_models += the models with info == 0.
 *   iteration  pass k = 1, 2, ...:  t' = (1 + sqrt(1 + 4 t^2)) / 2;  V = W + ((t - 1) / t') (W - W_prev), rounded to fp32;
 *              G = X~^T (softmax(X~ V) - Y) + lambda D V;  dV = -A^-1 G;  W_new = V + dV;  if <G, W_new - W> > 0 then
 *              t = 1 (gradient restart) else t = t'.  A model is done when max|dV| <= tol max(1, max|W_new|); a done
 *              model is frozen -- its blocks exit at once in later launches -- so its result depends neither on the
 *              other models nor on how often the caller looks at the status.  Reaching max_iter is not an error:
 *              converged stays 0.
 *   gae_logreg_pass: grid (slabs, tiles of 4 models).  Each fold's list is cut into chunks of GAE_LOGREG_CHUNK_ROWS rows
 *              (a chunk never straddles folds); a slab is GAE_LOGREG_SLAB_CHUNKS consecutive chunks of the list, so the
 *              number of slabs, ceil((ceil(n_rows / chunk) + folds) / slab), is a function of the list sizes alone.  A
 *              block stages a chunk once in LDS, x~ formed in fp32 by one rounded subtraction, and uses it for every
 *              model of its tile.  Logits on v_mfma_f32_16x16x4_f32 (d + 1 and c padded with zeros to the tile; a wave
 *              owns whole output tiles, the summed index is never split); the row softmax in fp32: max, subtract, exp,
 *              ascending sum, one reciprocal, each probability the product with it; the residual subtracts the one-hot
 *              label; the chunk's gradient R^T X~ on the same instruction, accumulated in fp32 over the slab's chunks in
 *              ascending order.  A chunk of fold f is skipped, not masked, for model f.  One partial per (slab, model).
 *              GAE_LOGREG_EVAL: the same staging and product at V (after a fit: fp32 of the final W), then per row in fp64
 *              the negative log-likelihood log sum exp(z - max) - (z_y - max) and the test arg max == y (ties to the
 *              lower class), for fold model m over its OWN fold and for the all-rows model over every row: nll fp64
 *              [models] and correct int64 [models] (NaN / 0 where the model failed), rows added in ascending order, slabs
 *              in THE order of partial lists.
 *   gae_logreg_update: one block per model, after the pass of the same models.  The slab partials are added in fp64 in
 *              THE order of partial lists (csrc/common.h sum_partials: <= 32 one lane in order; more: 64 lanes, lane l
 *              adds l, l + 64 ..., then the shuffle-down tree); + lambda D V; the c systems are solved with the stored
 *              factor; the restart test and the stopping rule run in fp64 in a fixed order (per thread ascending, then a
 *              fixed tree).  At a stop (done, or iteration == max_iter) V = fp32(W), coef fp64 [models][c][d] and
 *              intercept fp64 [models][c] are written, the intercept mapped back through the pivot in fp64
 *              (b = W[k][0] - sum_j p_j W[k][1 + j]), n_iter = iteration, converged = done, status.active_models -= 1.
 *              Because W starts at 0 and every update sums to zero over the classes, the parameters sum to (about) zero
 *              over the classes: the minimum-norm representative of the shift-invariant intercepts.
 *   status     a 32-byte device block the caller zeroes: active_models (see above), nonfinite_rows (gae_logreg_predict),
 *              errors: GAE_LOGREG_ERR_FOLD_PTR (fold_ptr not monotone from >= 0 to n_rows: nothing is read through it),
 *              _ROW_ID (a row id outside [0, n): skipped), _LAMBDA, _LABEL, _NONFINITE (a model's gradient or iterate
 *              left the finite numbers -- a non-finite feature in a listed row does that; info = -3).
 *   workspace  gae_logreg_workspace_bytes(n_rows, d, c, folds, n_lambdas, model_batch): a pure host function, positive,
 *              non-decreasing in n_rows, in the model count and in model_batch.  The same block, with the same arguments,
 *              is passed to every call of a fit: it holds the factors and the iteration state, then one launch's partials.
 *   No float atomics: the result has the same bits run to run, for any ldx, any stream and any cut of the models.
 * gae_logreg_predict: labels int32 [n] (arg max, ties to the lower class) and, when proba is not NULL, fp32 [n, c] rows
 * ldp apart, of the model (coef fp64 [c][d], intercept fp64 [c]) through the pass kernel's staging, product and softmax
 * code about `pivot`.  A row that holds a non-finite feature gives -1 / NaN and adds to status.nonfinite_rows.
 * Argument errors are returned before anything is dereferenced or launched (no GPU is needed to see them). */
enum { GAE_LOGREG_CHUNK_ROWS = 64, GAE_LOGREG_SLAB_CHUNKS = 8 };
enum { GAE_LOGREG_EVAL = 1 };
enum { GAE_LOGREG_ERR_FOLD_PTR = 1, GAE_LOGREG_ERR_ROW_ID = 2, GAE_LOGREG_ERR_LAMBDA = 4, GAE_LOGREG_ERR_LABEL = 8,
       GAE_LOGREG_ERR_NONFINITE = 16 };

typedef struct gae_logreg_status {
    int64_t active_models, nonfinite_rows, errors, reserved;
} gae_logreg_status;

int64_t gae_logreg_workspace_bytes(int64_t n_rows, int64_t d, int64_t c, int64_t folds, int64_t n_lambdas,
                                   int64_t model_batch);

int gae_logreg_factor(const double *stats, int64_t d, int64_t c, int64_t folds, const double *lambdas, int64_t n_lambdas,
                      int64_t n_rows, int64_t model_batch, double *coef, double *intercept, int32_t *info, int32_t *n_iter,
                      int32_t *converged, gae_logreg_status *status, void *workspace, int64_t workspace_bytes, void *stream);

int gae_logreg_pass(const float *X, int64_t ldx, const int32_t *y, int64_t n, int64_t d, int64_t c, const float *pivot,
                    const int32_t *rows, int64_t n_rows, const int32_t *fold_ptr, int64_t folds, int64_t n_lambdas,
                    int64_t model_batch, int64_t model_lo, int64_t model_count, int flags, double *nll, int64_t *correct,
                    gae_logreg_status *status, void *workspace, int64_t workspace_bytes, void *stream);

int gae_logreg_update(int64_t d, int64_t c, int64_t folds, const double *lambdas, int64_t n_lambdas, int64_t n_rows,
                      int64_t model_batch, int64_t model_lo, int64_t model_count, int64_t iteration, int64_t max_iter,
                      double tol, const float *pivot, double *coef, double *intercept, int32_t *info, int32_t *n_iter,
                      int32_t *converged, gae_logreg_status *status, void *workspace, int64_t workspace_bytes, void *stream);

int gae_logreg_predict(const float *X, int64_t ldx, int64_t n, int64_t d, int64_t c, const double *coef,
                       const double *intercept, const float *pivot, int32_t *labels, float *proba, int64_t ldp,
                       gae_logreg_status *status, void *stream);

/* ---- K29: exact t-SNE of an embedding into the plane (ops.tsne, ops.tsne_affinities, GAE.map_nodes, GAE.map_graphs)
 * The 2-D map of a latent space -- the Cora figure of the GAE / VGAE papers -- without an n x n matrix and without
 * float atomics.  Definitions are sklearn's:
 *   Y fp32 [n, 2], rows ldy >= 2 floats apart (any ldy; what lies between the rows is never read)
 *   q_ij = 1 / (1 + |y_i - y_j|^2),  Z = sum_{i != j} q_ij,  P sparse, symmetric, sum P = 1 (a CSR with int32 indptr)
 *   g_i = 4 (alpha sum_j P_ij q_ij (y_i - y_j) - (1 / Z) sum_{j != i} q_ij^2 (y_i - y_j)),  alpha the exaggeration
 *   gain_c += 0.2 where sign(g_c) != sign(v_c) (sign in {-1, 0, 1}), else gain_c *= 0.8; then gain_c = max(gain_c, 0.01)
 *   v = mu v - eta gain g;  y += v.  No recentring.
 *   KL = sum_{P_ij > 0} P_ij log(P_ij Z / q_ij) = sum P log P + log Z sum P + sum P log(1 + d^2): the status block
 *   carries the last two pieces, the caller owns the first.
 * INIT (gae_tsne_init): y[i][c] = (2 u - 1) 1e-4f in fp32, u = (w >> 8) 2^-24, w = word 0 of philox4x32_10(ctr = 2 i + c,
 *   draw = 0, key = seed ^ GAE_TSNE_KEY_XOR): 2 u - 1 is exact, the product rounds once.
 * AFFINITIES (gae_tsne_affinities): neighbour lists index int32 [n, k] / dist2 fp32 [n, k] (rows ld apart; gae_knn's
 *   output) -> p_out fp32 [n, k] (ldp), p_{j|i} = exp(-beta_i (D_ij - D_i,min)) / sum, and perplexity_out fp64 [n], the
 *   perplexity each row reached, exp(H_i) with H_i = log S + beta T / S, S = sum e, T = sum (D - D_min) e.  An entry is
 *   a neighbour when index >= 0 and dist2 is finite; other entries get p = 0.  All arithmetic is fp64, one wave per
 *   row, lane l holds entry l, wave sums by the xor butterfly 32, 16, ..., 1.  beta is found by
 *   GAE_TSNE_BISECT_ITERS = 100 steps from beta = 1 on the bracket [0, open): H > log(perplexity) -> lo = beta, beta =
 *   2 beta while the bracket is open, else (beta + hi) / 2; otherwise hi = beta, beta = (lo + beta) / 2; p is evaluated
 *   at the beta the last step leaves.  A row whose entropy cannot reach the target (ties at the minimum, all-equal
 *   distances) ends at the limit distribution: uniform over the tied minima / over the row.  A row with fewer than
 *   2 neighbours gets p = 1 on its neighbour (perplexity_out = the neighbour count).
 * CHUNKS  gae_tsne_chunk(n) = 256 for n <= 8192, 1024 for n <= 32768, 8192 beyond: a pure host function of n, never of the
 *   device, the grid or a knob.  Chunk c owns the columns [c chunk, min((c + 1) chunk, n)).
 * REPULSION (gae_tsne_repulsion; the hot path): for every row i and every chunk c in [chunk_lo, chunk_hi) one partial
 *   (fx, fy, z) at workspace floats [(3 c + {0, 1, 2}) n + i] -- the partials are the FIRST region of the workspace --,
 *   each an fp32 chain from 0.f over the chunk's j ascending, j = i left out by predicate:
 *     dx = y_ix - y_jx; dy = y_iy - y_jy; d2 = fmaf(dy, dy, dx * dx); q = rcp(1.0f + d2);
 *     z += q; fx = fmaf(q * q, dx, fx); fy = fmaf(q * q, dy, fy)
 *   rcp is v_rcp_f32 (1 ulp; exact at 1.0f, so a duplicated row adds exactly 1 to z and 0 to the force), not an IEEE
 *   division.  Columns and rows past n are clamped for loads and never added or stored.  Nothing is written per pair.
 *   Any cut of [0, chunks) into calls gives the same bits.
 * UPDATE (gae_tsne_update): two launches.  reduce: a row's chunk partials in the library's one order for partial
 *   lists (common.h sum_partials: one lane for <= 32 chunks, 64 lanes beyond); the attraction over the row's CSR entries
 *   e ascending, fp32 chains from 0.f: w = P_e / (1.0f + d2) (IEEE division), ax = fmaf(w, dx, ax), ay likewise (dx, dy, d2
 *   as above); the row's KL term sum_e P_e log1p(d2) in fp64; the rows' z of a block of 256 rows (4 rows beyond 32
 *   chunks) in sum_partials' order, one Z partial per block.  update: Z = the block partials in sum_partials' order;
 *   g_c = 4.0f * fmaf(alpha, a_c, -(r_c * (1.0f / Z))); the gain rule; v = fmaf(mu, v, -((eta * gain) * g)); y += v.
 *   velocity and gains are dense fp32 [n, 2], the caller's state (zeros and ones before the first iteration).
 *   alpha, mu, eta are rounded to fp32 once.  tsne.hip is compiled without contraction: the products above are fused
 *   exactly where fmaf is written.
 *   status       a 64-byte device block, zeroed by the caller before the first iteration:
 *                  done        set when sqrt(grad2) <= min_grad_norm; every kernel of a later iteration then returns at
 *                              once: iterations may be enqueued in groups and the block read once per group
 *                  iteration   += 1 per update that ran
 *                  nonfinite   += the rows whose new y is not finite
 *                  ticket      the library's (an integer ticket; 0 between calls)
 *                  p_log_d     sum P log(1 + d^2) of the Y on entry: fp64, per block of 256 rows a halving tree, the
 *                              blocks by thread t adding blocks t, t + 256, ... and the same tree
 *                  log_z, z    log Z (fp64 log of the fp32 Z) and Z
 *                  grad2       sum |g|^2, fp64, in the order of p_log_d
 * DETERMINISM  No float atomics.  The grids are functions of n alone: the same bits run to run, for any ldy, any
 *   stream, any grouping of the iterations and any cut of the chunks into calls.
 * WORKSPACE  gae_tsne_workspace_bytes(n, nnz): a pure host function; 12 n ceil(n / chunk) bytes of partials plus O(n).
 *   A call whose partials would exceed GAE_TSNE_MAX_WORKSPACE = 2^33 bytes is GAE_E_SIZE, not a fallback.
 * Argument errors are returned before any launch and need no GPU: negative sizes, n or nnz >= 2^31, update with n < 2
 *   (GAE_E_SIZE); k outside 1..64, perplexity < 1 or >= k, a chunk range outside [0, chunks], exaggeration <= 0, momentum
 *   outside [0, 1), learning_rate <= 0, NaN min_grad_norm (GAE_E_RANGE); ld / ldp < k, ldy < 2 (GAE_E_SIZE); NULL
 *   pointers (GAE_E_NULL); a short workspace (GAE_E_WORKSPACE). */
enum { GAE_TSNE_MAX_K = 64, GAE_TSNE_BISECT_ITERS = 100 };
#define GAE_TSNE_KEY_XOR 0x2545F4914F6CDD1DULL
#define GAE_TSNE_MAX_WORKSPACE (1LL << 33)

typedef struct gae_tsne_status {
    int64_t done, iteration, nonfinite, ticket;
    double p_log_d, log_z, grad2, z;
} gae_tsne_status;

int64_t gae_tsne_chunk(int64_t n);

int64_t gae_tsne_workspace_bytes(int64_t n, int64_t nnz);

int gae_tsne_init(float *Y, int64_t ldy, int64_t n, uint64_t seed, void *stream);

int gae_tsne_affinities(const int32_t *index, const float *dist2, int64_t ld, int64_t n, int64_t k, double perplexity,
                        float *p_out, int64_t ldp, double *perplexity_out, void *stream);

int gae_tsne_repulsion(const float *Y, int64_t ldy, int64_t n, int64_t chunk_lo, int64_t chunk_hi,
                       const gae_tsne_status *status, void *workspace, int64_t workspace_bytes, void *stream);

int gae_tsne_update(float *Y, int64_t ldy, int64_t n, const int32_t *indptr, const int32_t *indices, const float *P,
                    int64_t nnz, float *velocity, float *gains, double exaggeration, double momentum,
                    double learning_rate, double min_grad_norm, gae_tsne_status *status, void *workspace,
                    int64_t workspace_bytes, void *stream);

/* ---- K31: principal components of a frozen feature (ops.pca, ops.pca_transform, GAE.pca_nodes, GAE.pca_graphs)
 * An fp64 symmetric eigensolver in one block plus one projection pass.  No float atomics, no libm: the same bits run to
 * run, for any ldx and any stream.  pca.hip is compiled without contraction; nothing below is fused unless fma is written.
 * SOLVE (gae_pca_solve): one launch of ONE block.
 *   stats        ONE fold's packed upper triangle as gae_ridge_stats writes it, width W = 1 + d + t; the t trailing rows
 *                and columns are ignored.  pivot: the fp32 [>= d] one the moments were taken with, or NULL = zeros.
 *                n_rows_used: the length of the list the moments were taken over (checked on the host: 0 .. 2^31 - 1;
 *                the device takes the count c from the moments themselves).
 *   centring     c = S[0][0], s_j = S[0][1 + j], mu_j = s_j / c;  for i <= j: C_ij = C_ji = (S_xx[i][j] - s_j mu_i) / (c - 1)
 *                (sklearn's n - 1 denominator);  mean[j] = (double)pivot[j] + mu_j.
 *   Jacobi       cyclic, two-sided, on the full symmetric C in LDS; V (as V^T, starting from I) beside it for d <= 96,
 *                else in the workspace: the bits do not depend on which.  dp = d rounded up to even, m = dp / 2.  A sweep
 *                is the dp - 1 rounds r = 0 .. dp - 2 of the round-robin tournament: pair 0 = {r, dp - 1}, pair k =
 *                {(r + k) mod (dp - 1), (r - k) mod (dp - 1)}, k = 1 .. m - 1; p = the smaller index, q = the larger.  For
 *                odd d index dp - 1 does not exist: its partner r sits the round out (a pair that is not rotated).
 *   rotation     of the pair (p, q), from the matrix at the start of the round: it is skipped when a_pq == 0 or
 *                |a_pq| <= 2^-53 sqrt(|a_pp| |a_qq|).  Otherwise tau = (a_qq - a_pp) / (2 a_pq), t = sgn(tau) / (|tau| +
 *                sqrt(1 + tau tau)) (sgn(0) = +1), c = 1 / sqrt(1 + t t), s = t c; every +, -, x, /, sqrt a single
 *                correctly rounded fp64 operation in the order written.  A skipped pair has c = 1, s = 0.
 *   a round      A <- J^T A J for J the product of the round's disjoint rotations, in 2 x 2 blocks: for pairs k < l
 *                ((p, q) with c1, s1 and (r, u) with c2, s2) FIRST the column rotation x' = c2 x - s2 y, y' = s2 x + c2 y on
 *                (x, y) = (a_pr, a_pu) and (a_qr, a_qu), THEN the row rotation x' = c1 x - s1 y, y' = s1 x + c1 y on the
 *                results (a'_pr, a'_qr) and (a'_pu, a'_qu); each product rounded, then the sum.  The block's transpose is a
 *                copy, so A stays symmetric bit for bit.  A pair's own block: a_pp -= t a_pq, a_qq += t a_pq, a_pq = a_qp
 *                = 0 (untouched when skipped).  V^T rows p, q take the row rotation.  Threads split blocks and columns,
 *                never a sum.
 *   stopping     after the first sweep that rotates nothing (info 0), or after GAE_PCA_MAX_SWEEPS sweeps (info 1).
 *   ordering     eigenvalues = the final diagonal, descending; equal values to the lower index of the diagonal (a NaN, which only
 *                non-finite moments give, sorts last).  The first
 *                n_components go out: values fp64 [k] as computed (a tiny negative value is reported, not clamped),
 *                components fp64 [k][d] = the columns of V; the entry of largest magnitude of each is made positive (ties
 *                to the lower index) by negating the row: sklearn's v-based svd_flip.
 *   status       a 64-byte device block.  gae_pca_solve WRITES info, n_sweeps (sweeps run, the one that rotated nothing
 *                included), n_rotations, off_norm = sqrt(sum_i (sum_{j != i} a_ij a_ij)) (j, then i ascending) and
 *                total_variance = the sum of all d eigenvalues in their output order; gae_pca_transform ADDS to
 *                nonfinite_rows, nonpositive_components and errors (integer atomics).
 *   info         0 converged; 1 the sweep cap was reached; -1 c < 2 (fewer than two rows).  Where info != 0 mean, values,
 *                components, off_norm and total_variance are NaN.
 *   workspace    gae_pca_workspace_bytes(d) bytes: a pure host function of d, positive; GAE_E_RANGE for d outside 1..128.
 * PROJECT (gae_pca_transform): Z[i][c] = sum_j (x_ij - m_j) v_cj, fp32 [n_rows, k], rows ldz >= k apart.  m and v are
 *   rounded to fp32 once, the subtraction is one fp32 operation, the sum one fp32 fma chain from +0 over j ascending on
 *   v_mfma_f32_16x16x4_f32 (K27's chains; the padding of j and c to tiles adds exact zeros).  GAE_PCA_WHITEN: then one fp32
 *   product by (float)(1 / sqrt(values[c])), the fp64 quotient of the fp64 root; a component whose value is not > 0 gives
 *   score 0 and is counted once in nonpositive_components.  rows: int32 [n_rows] ids or NULL = rows 0 .. n - 1 (then n_rows
 *   == n); rows that are not listed are never read.  A listed row holding a non-finite value gives a NaN row and is
 *   counted in nonfinite_rows; a row id outside [0, n) gives a NaN row and sets GAE_PCA_ERR_ROW_ID.  X is streamed once.
 * Argument errors are returned before any launch and need no GPU: d outside 1..128, n_components outside 1..d, t outside
 *   0..8, unknown flag bits (GAE_E_RANGE); negative sizes, n or n_rows >= 2^31, ldx < d, ldz < k, rows = NULL with n_rows
 *   != n (GAE_E_SIZE); NULL pointers -- values only under GAE_PCA_WHITEN, X only with n_rows > 0 -- (GAE_E_NULL); a short
 *   workspace (GAE_E_WORKSPACE). */
enum { GAE_PCA_MAX_D = 128, GAE_PCA_MAX_SWEEPS = 30 };
enum { GAE_PCA_WHITEN = 1 };
enum { GAE_PCA_ERR_ROW_ID = 1 };

typedef struct gae_pca_status {
    int64_t info, n_sweeps, n_rotations, nonfinite_rows, nonpositive_components, errors;
    double off_norm, total_variance;
} gae_pca_status;

int64_t gae_pca_workspace_bytes(int64_t d);

int gae_pca_solve(const double *stats, int64_t d, int64_t t, const float *pivot, int64_t n_rows_used, int64_t n_components,
                  int flags, double *mean, double *values, double *components, gae_pca_status *status, void *workspace,
                  int64_t workspace_bytes, void *stream);

int gae_pca_transform(const float *X, int64_t ldx, int64_t n, int64_t d, const int32_t *rows, int64_t n_rows,
                      const double *mean, const double *components, const double *values, int64_t k, int flags, float *Z,
                      int64_t ldz, gae_pca_status *status, void *stream);

/* ---- K32: spectral embedding of a graph (ops.spectral_embedding): the k algebraically largest eigenpairs of
 * S = D^-1/2 (A + sigma I) D^-1/2 by Chebyshev-filtered block subspace iteration with a Rayleigh-Ritz step, in fp64.
 * No float atomics, no rocSOLVER / rocSPARSE, no host linear algebra: the same bits run to run, for any stream and any
 * grid.  spectral.hip is compiled without contraction; a product and a sum are fused exactly where fma is written.
 * The host drives the launches (ops/spectral.py); everything it needs between them stays on the device.
 * OPERANDS   tall blocks fp64 [n][b], row-major, rows b apart, 16-byte aligned; b even, 2 <= b <= 128; 1 <= k <= 64, k <= b;
 *            n < 2^31.  CSR: int32 indptr [n + 1], int32 indices [nnz] (graph.csr()); a duplicate edge counts once per
 *            copy; an index outside [0, n) is skipped and sets GAE_SPECTRAL_ERR_INDEX.
 * SCALE      (gae_spectral_scale) deg_i = indptr[i + 1] - indptr[i]; t = (double)deg_i + sigma; s_i = t > 0 ? 1 / sqrt(t) : 0.
 * INIT       (gae_spectral_init) element e = i b + c of V: block q = e >> 2 is philox4x32_10(ctr = q, draw = 0, key = seed ^
 *            GAE_SPECTRAL_KEY_XOR) (csrc/common.h); the pair h = (e >> 1) & 1 of the block has u1 = ((w[2h] >> 8) + 0.5) 2^-24,
 *            u2 = (w[2h + 1] >> 8) 2^-24 (exact in fp64), rad = sqrt(-2 log(u1)), ang = 6.283185307179586 u2; the even element is
 *            rad cos(ang), the odd one rad sin(ang) (fp64 library functions: a few ulp, not restated bit for bit).
 * PRODUCT    (gae_spectral_spmm) for every row i and column c, coef = {alpha, beta, gamma} read from the DEVICE:
 *              acc = +0;  for e = indptr[i] .. indptr[i + 1] - 1 ascending, j = indices[e]: acc = fma(s_j, Yin[j][c], acc);
 *              sigma != 0: acc = fma(sigma s_i, Yin[i][c], acc)   (sigma s_i one rounded product);
 *              t = s_i acc;  o = alpha t;  o = fma(beta, Yin[i][c], o);  Yprev != NULL: o = fma(gamma, Yprev[i][c], o);
 *              Yout[i][c] = o.
 *            A row goes to a group of lanes that split the columns in 16-byte pairs, never the sum.  Yout must not
 *            alias Yin; it may alias Yprev.
 * GRAM       (gae_spectral_gram) G = V^T V and H = V^T AV, both written as full symmetric [b][b] matrices from their computed
 *            upper triangles.  Rows go in chunks of GAE_SPECTRAL_CHUNK_ROWS = 256; a chunk's sums run on
 *            v_mfma_f64_16x16x4_f64, four rows a step, rows ascending; the chunk partials are added in the library's one
 *            order for partial sums (common.h: <= 32 partials one lane in order, more 64 lanes and the fixed tree).
 *            max_blocks > 0 caps the grid (blocks then walk chunks b, b + grid, ...): the bits do not depend on it.
 * SOLVE      (gae_spectral_solve) three launches of ONE block each; every -, x, / and sqrt one rounded operation:
 *   factor     G = L L^T by cholesky.h's Cholesky-Crout (column j: piv = g_jj - sum_{k<j} l_jk l_jk, l_ij = (g_ij - sum_{k<j}
 *              l_ik l_jk) / sqrt(piv), k ascending, each product subtracted as it is formed), from the lower triangle.
 *   reduce     X = L^-1 H: column c, i ascending: x = h_ic; k < i ascending: x = x - l_ik x_kc; x_ic = x / l_ii.
 *              H' = X L^-T: row r, j ascending: y = x_rj; k < j ascending: y = y - l_jk y_rk; y_rj = y / l_jj.  The upper
 *              triangle (r <= j) is H'; the lower one is its copy.
 *   Jacobi     gae_pca_solve (K31) as it stands, on a packed triangle of width 1 + b with S[0][0] = 2, S[0][1..] = 0, S_xx =
 *              H', pivot = NULL, t = 0: its centring returns H' bit for bit ((S - 0 . 0) / 1).  theta [b] = its values
 *              (descending), W = its components (row c = vector c, K31's sign rule).
 *   back       T = L^-T W^T: column c, i descending: x = w_ci; k = i + 1 .. b - 1 ascending: x = x - l_ki t_kc; t_ic = x / l_ii.
 *              T fp64 [b][b] row-major, theta and the filter's coefficients go to the workspace, theta also to values.
 *   filter     a = max(min(theta_b, theta_k - 0.02), -0.5);  e = (a + 1) 0.5;  c = (a - 1) 0.5;  s1 = e / (theta_1 - c);
 *              coef[0] = {1, 0, 0} (the plain product);  coef[1] = {s1 / e, -(c alpha), 0};  s = s1;  for d = 2 .. degree:
 *              s2 = 1 / (2 / s1 - s);  alpha = (2 s2) / e;  coef[d] = {alpha, -(c alpha), -(s s2)};  s = s2.
 *              Degree d of the filter is the PRODUCT with coef[d], Yprev = NULL at d = 1 (Zhou & Saad's scaled Chebyshev
 *              recurrence on [-1, a], scaling point theta_1).
 *   info       0; j >= 1: the Cholesky met pivot j <= 0 or not finite; -1: the Jacobi reached its sweep cap; -2: a Ritz
 *              value is not finite.  Where info != 0, T and theta are NaN.
 * ROTATE     (gae_spectral_rotate) V <- V T and AV <- AV T in place, row by row: out[i][c] = the fma chain from +0 over j
 *            ascending of in[i][j] T[j][c].  Residual: d = AV'[i][c] - theta_c V'[i][c] (product rounded, then the difference),
 *            chunk partial = the sum over the chunk's rows ascending of d d from +0; the partials of a column are added in
 *            the library's one order; res_c = sqrt(sum).  n_converged = the longest prefix of the first k columns with res_c
 *            <= tol.  A non-finite res_c among the first k sets nonfinite.
 * FINISH     (gae_spectral_finish) column c of the output is column first + c of V.  The entry of largest magnitude of a
 *            column (chunks of 256 rows ascending, rows ascending, a later entry wins only when strictly larger) is made
 *            positive by negating the column.  vectors fp64 [n][k]; embedding fp32 [n][k] = (float) of the vector entry
 *            times s_i (GAE_SPECTRAL_SCALE_DEGREE) or times sqrt(max(theta_c, 0)) (GAE_SPECTRAL_SCALE_VALUE), one fp64 product.
 * STATUS     a 64-byte device block the host reads once per checked iteration; n_spmm counts PRODUCT launches.
 * WORKSPACE  gae_spectral_workspace_bytes(n, nnz, b): a pure host function; one carve serves every entry point.
 * Argument errors are returned before any launch and need no GPU: b odd or outside 2..128, k outside 1..min(b, 64), degree
 *   outside 1..GAE_SPECTRAL_MAX_DEGREE, unknown scaling, sigma < 0 or tol < 0 or not finite (GAE_E_RANGE); n < 1 or n >= 2^31,
 *   nnz < 0 or nnz >= 2^31, first + k > b, negative max_blocks, Yout aliasing Yin, AV aliasing V, a tall operand off a 16-byte
 *   boundary (GAE_E_SIZE); NULL pointers (GAE_E_NULL); a short workspace (GAE_E_WORKSPACE). */
enum { GAE_SPECTRAL_MAX_B = 128, GAE_SPECTRAL_MAX_K = 64, GAE_SPECTRAL_MAX_DEGREE = 12, GAE_SPECTRAL_CHUNK_ROWS = 256 };
enum { GAE_SPECTRAL_SCALE_NONE = 0, GAE_SPECTRAL_SCALE_DEGREE = 1, GAE_SPECTRAL_SCALE_VALUE = 2 };
enum { GAE_SPECTRAL_ERR_INDEX = 1 };
#define GAE_SPECTRAL_KEY_XOR 0x5851F42D4C957F2Dull

typedef struct gae_spectral_status {
    int64_t info, n_converged, n_spmm, nonfinite, errors;
    double theta_1, theta_k, res_max;      /* res_max: the largest residual of the first k columns */
} gae_spectral_status;

int64_t gae_spectral_workspace_bytes(int64_t n, int64_t nnz, int64_t b);

int gae_spectral_scale(const int32_t *indptr, int64_t n, double sigma, double *s, void *stream);

int gae_spectral_init(double *V, int64_t n, int64_t b, uint64_t seed, void *stream);

int gae_spectral_spmm(const int32_t *indptr, const int32_t *indices, int64_t n, int64_t nnz, const double *s, double sigma,
                      const double *Yin, const double *Yprev, double *Yout, int64_t b, const double *coef_dev,
                      gae_spectral_status *status, void *stream);

int gae_spectral_gram(const double *V, const double *AV, int64_t n, int64_t b, double *G, double *H, int64_t max_blocks,
                      void *workspace, int64_t workspace_bytes, void *stream);

int gae_spectral_solve(const double *G, const double *H, int64_t b, int64_t k, int64_t degree, double *T, double *values,
                       double *coef, gae_spectral_status *status, void *workspace, int64_t workspace_bytes, void *stream);

int gae_spectral_rotate(double *V, double *AV, int64_t n, int64_t b, int64_t k, const double *T, const double *values,
                        double tol, double *residuals, gae_spectral_status *status, void *workspace,
                        int64_t workspace_bytes, void *stream);

int gae_spectral_finish(const double *V, int64_t n, int64_t b, int64_t first, int64_t k, const double *values, const double *s,
                        int scaling, double *vectors, float *embedding, void *workspace, int64_t workspace_bytes,
                        void *stream);

/* ---- K33: circular fingerprints of the member graphs of a resident molecule set (ops.fingerprint_graphs)
 * A Morgan / Weisfeiler-Lehman fingerprint on what the set stores: the featuriser rows as atom invariants, the
 * block-diagonal CSR as neighbourhoods.  The set holds no bond orders, so the bits are NOT RDKit's ECFP: the same family
 * of descriptor, not the same numbers.  All arithmetic is uint64 and wrapping; no float is used anywhere.
 *   mix(x)     the splitmix64 finaliser: x ^= x >> 30; x *= 0xbf58476d1ce4e5b9; x ^= x >> 27; x *= 0x94d049bb133111eb;
 *              x ^= x >> 31.   GOLD = 0x9e3779b97f4a7c15.
 *   RADIUS 0   h = GOLD; for f = 0 .. f_in - 1 ascending: h = mix(h ^ bits_f); id_0(v) = h.  bits_f is the fp32 bit pattern
 *              of feature f of atom v, zero-extended, -0.0 taken as +0.0; a GAE_U8 feature contributes the pattern of its
 *              value as fp32 (the same fingerprints in either storage); non-finite values hash by their bits.
 *   RADIUS r   id_r(v) = mix(mix(id_{r-1}(v) + r GOLD) + sum_u mix(id_{r-1}(u))), u over the entries of v's CSR row (a
 *              duplicate entry counts twice; a column outside the graph's own node range is skipped).  The sum commutes:
 *              the result does not depend on the order of the row, the edge list or the atoms.
 *   EMISSION   every (v, r), 0 <= r <= radius, contributes slot id_r(v) mod n_bits.  counts = 0: the bit is set; out is
 *              int32 words [n_out, n_bits / 32], bit j of word w is slot 32 w + j.  counts = 1: the slot is incremented;
 *              out is int32 [n_out, n_bits].  Structurally duplicate neighbourhoods are not removed.
 * Row k of out belongs to graph graph_ids[k] (NULL: graph k; any order, repeats allowed); rows are ldo int32 apart and
 * only their first n_bits / 32 (or n_bits) columns are written: they are zeroed here, on the caller's stream.
 * One launch per radius; launch r reads id_{r-1} from, and writes id_r to, the workspace (two uint64 arrays indexed by
 * global node id).  Integer atomicOr / atomicAdd only: the same bits run to run.  Work is proportional to the atoms of
 * the listed graphs; a graph of any size is walked in strides (0 nodes: a zero row).
 * SAFETY  a graph id outside [0, n_graphs) or a node range outside [0, n_nodes] gives a zero row; a row pointer outside
 * [0, n_edges] reads as an empty row: nothing outside the arrays is read or written.
 * feat: [n_nodes, f_in] of feat_dtype GAE_F32 or GAE_U8, rows ldf elements apart, no alignment asked.
 * radius 0 .. 8, n_bits a power of two in 64 .. 2048 (else GAE_E_RANGE), f_in >= 1, n_nodes, n_edges < 2^31 (GAE_E_SIZE).
 * Argument errors are returned before anything is dereferenced or launched: the above, an unknown feat_dtype
 * (GAE_E_DTYPE), ldf < f_in or ldo below the row width (GAE_E_SIZE), NULL graph_ptr / indptr / feat (n_nodes > 0) /
 * indices (n_edges > 0) / out (n_out > 0) / workspace (GAE_E_NULL), a short workspace (GAE_E_WORKSPACE). */
int64_t gae_fingerprint_workspace_bytes(int64_t n_nodes);

int gae_fingerprint_graphs(const int64_t *graph_ptr, int64_t n_graphs, int64_t n_nodes, int64_t n_edges,
                           const int32_t *indptr, const int32_t *indices, const void *feat, int feat_dtype, int64_t ldf,
                           int64_t f_in, const int64_t *graph_ids, int64_t n_out, int radius, int64_t n_bits, int counts,
                           int32_t *out, int64_t ldo, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- K34: exact Tanimoto k-nearest-neighbour search over bit fingerprints (ops.tanimoto_knn)
 * For every query row of Q int32 [m, n_words] (rows ldq words apart) the k rows of the database X int32 [n, n_words]
 * (ldx) of the largest Tanimoto similarity, without the m x n matrix.  Rows are read in place; no alignment is asked.
 * VALUE  a = popcount(q), b = popcount(x), c = popcount(q & x), u = a + b - c: the correctly rounded fp32 quotient
 *   float(c) / float(u), or 0.0f when u = 0.  For u <= 4096 (n_words <= 64) different fractions never share an fp32
 *   quotient and the quotients keep the exact order, so the order by value is the order by the exact fraction.
 * CANDIDATES of query i: every database row j in [0, n), minus j = i under GAE_KNN_EXCLUDE_SAME_INDEX (for Q = X).
 * ORDER OF A ROW  (value descending, j ascending).  Fewer than k candidates pad the tail with index -1 and value -inf.
 * DETERMINISM  No float atomics, ordinary launches only: the same bits run to run, for any ldq / ldx / ldo and `splits`.
 *   index_out int32 [m, ldo >= k], value_out fp32 [m, ldo >= k]: nothing beyond column k is written
 *   splits    column splits per group of 256 queries: 0 = auto, else 1 .. 16
 *   workspace at least gae_tanimoto_knn_workspace_bytes(m, n, n_words, k, splits) bytes: a pure host function, positive,
 *             non-decreasing in m, n, k and splits; a negative error code for a shape error.  O(n + m k splits) bytes
 * 1 <= n_words <= 64, 1 <= k <= 64 (else GAE_E_RANGE); 0 <= m, n < 2^31 (else GAE_E_SIZE).  Argument errors are returned
 * before anything is dereferenced or launched: the shape errors, splits outside 0..16, an unknown flag bit (GAE_E_RANGE),
 * ldq < n_words, ldx < n_words, ldo < k (GAE_E_SIZE), NULL index_out / value_out / Q (m > 0), NULL X (m, n > 0), NULL
 * workspace (GAE_E_NULL), a short workspace (GAE_E_WORKSPACE).
 * Launches: the database rows' bit counts, the sweep (k-best tail of csrc/topk_heap.h), the merge of the splits' lists. */
int64_t gae_tanimoto_knn_workspace_bytes(int64_t m, int64_t n, int64_t n_words, int64_t k, int splits);

int gae_tanimoto_knn(const int32_t *Q, int64_t ldq, int64_t m, const int32_t *X, int64_t ldx, int64_t n, int64_t n_words,
                     int64_t k, int flags, int splits, int32_t *index_out, float *value_out, int64_t ldo, void *workspace,
                     int64_t workspace_bytes, void *stream);

/* ---- K35 / K36: neighbourhood link-prediction baselines (ops.neighbour_scores, ops.neighbour_topk)
 * Common neighbours, Jaccard, Adamic-Adar, resource allocation and preferential attachment over a graph, without the
 * n x n two-hop matrix and without a float being accumulated anywhere.
 * GRAPH   the library's CSR: int32 indptr [n + 1], indices [nnz]; rows ascending, duplicates kept.  The graph must be
 *   SYMMETRIC (every edge listed in both directions); the wrapper checks, the kernels rely on it.  n < 2^30, nnz < 2^31.
 * NEIGHBOUR SETS  Gamma(i) is the set of DISTINCT columns of row i other than i: duplicate edges and self-loops do not
 *   count.  deg(i) = |Gamma(i)|.
 * PER PAIR (i, j)   common = |Gamma(i) & Gamma(j)|;  wsum_c = sum over w in Gamma(i) & Gamma(j) of W[w, c], for nw <= 2
 *   caller-supplied int64 weight columns W [n, nw] (row-major, dense).  The kernels know nothing about logarithms: they
 *   add integers.  i == j is allowed and gives common = deg(i).
 * WEIGHTS (built by the wrapper; the kernels take any int64)  fixed point with GAE_NEIGHBOUR_SCALE_BITS = 32 fraction
 *   bits, from a host table over the degrees 0 .. max degree in numpy fp64:  aa_q[d] = rint(2^32 / log(d)) for d >= 2, else
 *   0;  ra_q[d] = rint(2^32 / d) for d >= 1, else 0;  the table is gathered on the device by deg.  Every weight is below
 *   2^32.53 and common below 2^30, so every sum is below 2^63: overflow cannot happen.
 * SCORES (one stated operation each, formed by the wrapper)  cn = common;  jaccard = double(common) / double(deg_i +
 *   deg_j - common), 0 when the union is 0;  aa = double(aa_sum) * 2^-32, ra = double(ra_sum) * 2^-32;  pa = deg_i * deg_j
 *   (int64).
 * TOP-K  candidates of query row i: every j with j != i and common(i, j) >= 1, minus the j in Gamma(i) under
 *   GAE_NEIGHBOUR_EXCLUDE_EDGES.  kind: GAE_NEIGHBOUR_CN / _JACCARD / _AA / _RA (pa is not a local score: GAE_E_RANGE).
 *   ORDER  larger value first, then lower j (better() of csrc/topk_heap.h).  The value compared is the integer common (cn)
 *   or wsum (aa, ra: the one weight column w, node v's weight at w[v * ldw]) and the fp64 quotient for jaccard.  1 <= k <=
 *   64.  A row with fewer than k candidates pads its tail with index -1, common 0, wsum 0.
 *   ROUTES  a plan launch computes B_i = sum over w in Gamma(i) of rowlen(w) and lists the rows with 2 B_i <= table_slots
 *   as short (an LDS hash table keyed by j, integer LDS atomics, probes bounded by the table size), the others as long
 *   (windows of table_slots candidate columns with dense LDS accumulators, every Gamma(w) entered by binary search).
 *   The selection is by rank under the total order, so both routes, every table_slots and every run give the same bits.
 *   table_slots: 0 = GAE_NEIGHBOUR_TABLE_SLOTS, else a power of two in 64 .. 2048 (else GAE_E_RANGE).
 *   rows int32 [m] or NULL (then m rows: query q is node q).  index_out, common_out int32 [m, k], wsum_out int64 [m, k],
 *   dense.  deg int32 [n] from gae_neighbour_degrees.
 * STATUS  int64 [GAE_NEIGHBOUR_STATUS_WORDS] on the device, zeroed by the caller and read once at the end: word 0 the
 *   error bits or-ed in -- GAE_NEIGHBOUR_ERR_COLUMN (a column outside [0, n)), _ERR_ORDER (a row that is not ascending),
 *   _ERR_INDPTR (a row pointer outside [0, nnz] or descending), all three from gae_neighbour_degrees; _ERR_QUERY (a query
 *   index outside [0, n): that pair's common is -1, that row is padding), _ERR_TABLE (a full hash table: cannot happen on a
 *   graph without the other bits); words 1 and 2 the short and the long rows of the last gae_neighbour_topk.
 * SAFETY  a bad row pointer reads as an empty row, a bad column is never used as an index, every loop is bounded: nothing
 *   outside the arrays is read or written whatever the graph holds.
 * Argument errors are returned before anything is dereferenced or launched: negative sizes, n >= 2^30, nnz >= 2^31, m
 * beyond its range (GAE_E_SIZE); nw outside 0..2, k outside 1..64, an unknown kind or flag bit, a bad table_slots
 * (GAE_E_RANGE); NULL indptr / status / indices (nnz > 0) / deg (n > 0) / pairs and outputs (m > 0) / W (nw, n > 0) / w
 * (aa, ra) / workspace (GAE_E_NULL); a short workspace (GAE_E_WORKSPACE).  gae_neighbour_topk_workspace_bytes is a pure
 * host function, positive and non-decreasing in m: O(m) bytes, the two work lists. */
enum { GAE_NEIGHBOUR_SCALE_BITS = 32, GAE_NEIGHBOUR_TABLE_SLOTS = 1024, GAE_NEIGHBOUR_MAX_K = 64,
       GAE_NEIGHBOUR_MAX_WEIGHTS = 2, GAE_NEIGHBOUR_STATUS_WORDS = 4 };
enum { GAE_NEIGHBOUR_CN = 0, GAE_NEIGHBOUR_JACCARD = 1, GAE_NEIGHBOUR_AA = 2, GAE_NEIGHBOUR_RA = 3 };
enum { GAE_NEIGHBOUR_EXCLUDE_EDGES = 1 };
enum { GAE_NEIGHBOUR_ERR_COLUMN = 1, GAE_NEIGHBOUR_ERR_ORDER = 2, GAE_NEIGHBOUR_ERR_QUERY = 4, GAE_NEIGHBOUR_ERR_TABLE = 8,
       GAE_NEIGHBOUR_ERR_INDPTR = 16 };

int gae_neighbour_degrees(const int32_t *indptr, const int32_t *indices, int64_t n, int64_t nnz, int32_t *deg,
                          int64_t *status, void *stream);

int gae_neighbour_pairs(const int32_t *indptr, const int32_t *indices, int64_t n, int64_t nnz, const int32_t *pair_i,
                        const int32_t *pair_j, int64_t m, const int64_t *W, int64_t nw, int32_t *common_out,
                        int64_t *wsum_out, int64_t *status, void *stream);

int64_t gae_neighbour_topk_workspace_bytes(int64_t n, int64_t m);

int gae_neighbour_topk(const int32_t *indptr, const int32_t *indices, int64_t n, int64_t nnz, const int32_t *rows,
                       int64_t m, int64_t k, int kind, const int64_t *w, int64_t ldw, const int32_t *deg, int flags,
                       int64_t table_slots, int32_t *index_out, int32_t *common_out, int64_t *wsum_out, int64_t *status,
                       void *workspace, int64_t workspace_bytes, void *stream);

/* ---- K37 / K38: the DeepWalk baseline (ops.random_walks, ops.sgns_noise_table, ops.sgns_train, ops.deepwalk)
 * Uniform random walks over a CSR and a skip-gram trainer with negative sampling.  The trainer is SYNCHRONOUS mini-batch
 * Adagrad with negatives shared per walk -- DeepWalk-like, not a port of word2vec's asynchronous loop (which depends on
 * the order of its threads): every run gives the same bits, and a numpy restatement of this comment matches them.  No
 * n x n object is formed, no float atomic is used.  philox(ctr, draw, key) below is philox4x32_10 of csrc/common.h; word
 * i is its i-th 32-bit output.
 *
 * K37 gae_random_walks
 *   GRAPH  int64 indptr [n + 1], int32 indices [nnz], walked as stored: duplicate entries count with their multiplicity,
 *     a self-loop is stepped like any entry, a directed graph is walked along whatever the rows list (the library's
 *     graph.csr() lists, for a node, the SOURCES of its incoming edges: a walk steps against the edge direction; on a
 *     symmetric graph there is no difference).  n < 2^31; a row holds fewer than 2^32 entries.
 *   WALKS  starts int32 [m] or NULL (then m <= n and start s is node s); r = walks_per_start; L = length, 1 <= L <= 2^16;
 *     m r < 2^31.  walks int32 [m r, L], dense.  Walk id w = rep m + s (rep = 0 .. r - 1).  Position 0 is the start.  Step
 *     t >= 1 from node v: deg = indptr[v + 1] - indptr[v]; word = word (t & 3) of philox(w, GAE_DEEPWALK_WALK_DRAW + (t >>
 *     2), seed); the walk moves to indices[indptr[v] + ((uint64(word) deg) >> 32)].  Integers only.  deg = 0 ends the walk:
 *     the remaining positions are -1.
 *   STATUS  int64 [GAE_DEEPWALK_STATUS_WORDS], zeroed by the caller; word 0 the error bits: GAE_DEEPWALK_ERR_COLUMN (a
 *     column outside [0, n) was drawn: the walk ends there), _ERR_INDPTR (a row pointer outside [0, nnz], descending, or a
 *     row of 2^32 entries: read as an empty row), _ERR_START (a start outside [0, n): that walk is all -1).
 *
 * K38 gae_sgns_init / gae_sgns_walk_order / gae_sgns_accumulate / gae_sgns_update
 *   STATE  W (input table, the embedding) and C (context table), fp32 [n, d] dense; the Adagrad sums HW, HC fp32 [n, d];
 *     the accumulators AW, AC int64 [n, d], zero between batches (the caller zeroes them once, the update leaves zeros).
 *   LIMITS  1 <= d <= 128; 2 <= L <= 64; 1 <= window < L; M = shared_negatives in {16, 32, 48, 64}; 0 <= K = negatives <=
 *     1024; n, n_walks < 2^31; 0 <= epoch < 2^31: anything else is GAE_E_RANGE / GAE_E_SIZE, never another route.
 *   INIT  gae_sgns_init: element e of W (row-major) = (2 u - 1) bound in three fp32 operations (2 u, minus 1, times bound), u
 *     = float(word >> 8) 2^-24, word = word (e & 3) of philox(e >> 2, GAE_SGNS_INIT_DRAW, seed) (K27's draw).
 *   ORDER  gae_sgns_walk_order: order[p] = K27's keyed permutation of [0, n_walks) at position p of `epoch` (four Feistel
 *     rounds on 2 half bits, 4^half >= n_walks, round r: F = word 0 of philox((r << 32) | lo, 2^32 + epoch, seed); (hi, lo)
 *     <- (lo, hi ^ (F & mask)); cycle-walked until the value is below n_walks).  A batch is `count` consecutive positions
 *     from `first`.
 *   PER WALK w = order[position] of the batch (gae_sgns_accumulate):
 *   1 ROWS  ids = the walk's L nodes; a position is VALID when its id is not -1.  Ww = W[ids], Cw = C[ids]; an invalid
 *     position stands as a row of +0 (its coefficients are +0 as well: it never changes a chain of finite values).
 *   2 NEGATIVES  slot s = 0 .. M - 1: (w0, w1, w2, w3) = philox((epoch << 32) | w, GAE_SGNS_NEG_DRAW + (s >> 1), seed); u =
 *     (uint64(w[2 (s & 1) + 1]) << 32) | w[2 (s & 1)]; target = the high 64 bits of u cum[n]; neg[s] = the largest i of [0,
 *     n) with cum[i] <= target, by bisection (lo = 0, hi = n; mid = lo + ((hi - lo) >> 1); cum[mid] <= target moves lo, else
 *     hi; until hi - lo = 1).  cum int64 [n + 1] ascending from 0: a node of zero width is never drawn.  Cn = C[neg].
 *   3 LOGITS  S = Ww Cw^T (L x L), N = Ww Cn^T (L x M): every element ONE fp32 fma chain from +0 over the feature index
 *     ascending (v_mfma_f32_16x16x4_f32, K27's contract; the zero padding of d and L to 16 is exact).
 *   4 COEFFICIENTS  (p, j) is a positive iff 0 < |p - j| <= window and both positions are valid; c(p) = the positives of
 *     row p.  Gp[p, j] = float(sigma64(-double(S[p, j]))) on positives, +0 elsewhere.  coef(p) = float(K c(p)) / float(M),
 *     one fp32 division.  Gn[p, s] = -(coef(p) * float(sigma64(double(N[p, s])))), one fp32 product, and +0 where neg[s] ==
 *     ids[p] or p is invalid.  sigma64 is K30's sigma (its comment above; csrc/sigma64.h).  The M shared negatives weighted
 *     by K c(p) / M give every positive pair K negatives in expectation.
 *   5 GRADIENTS  fp32 fma chains from +0 again, masked terms staying in the chain with their +0 coefficient:  dW[p] over the
 *     contexts j ascending, then the negatives s ascending, of Gp[p, j] Cw[j] and Gn[p, s] Cn[s];  dCw[j] over p ascending of
 *     Gp[p, j] Ww[p];  dCn[s] over p ascending of Gn[p, s] Ww[p].
 *   6 SCATTER  every element x of dW, dCw (valid positions) and dCn becomes llrint(double(x) 2^32) (ties to even) and is added
 *     to AW[ids[p]], AC[ids[j]], AC[neg[s]] by a 64-bit integer atomic: exact and order-free; sums wrap as int64.  |x| >=
 *     2^20 or a non-finite x sets GAE_DEEPWALK_ERR_RANGE and is not added.
 *   UPDATE  gae_sgns_update, per element of W and of C whose accumulator a is not 0 (the others are untouched), single
 *     correctly rounded fp32 operations in this order:  g = float(double(a) 2^-32);  h = fmaf(g, g, h);  s = sqrtf(h) + eps;
 *     q = g / s;  x = fmaf(lr, q, x);  then a = 0.  (The gradient is that of the log-likelihood: the step ascends.)  A
 *     non-finite x or h sets GAE_DEEPWALK_ERR_NONFINITE.
 *   STATUS  the block of K37; further bits: _ERR_RANGE, _ERR_NONFINITE, _ERR_NODE (a walk-table entry outside [-1, n): read
 *     as -1), _ERR_ORDER (an order entry outside [0, n_walks): that walk is skipped).  The wrapper reads it once per epoch.
 * Argument errors are returned before anything is dereferenced or launched (GAE_E_SIZE, GAE_E_RANGE, GAE_E_NULL). */
enum { GAE_DEEPWALK_STATUS_WORDS = 4, GAE_DEEPWALK_MAX_LENGTH = 65536, GAE_SGNS_MAX_LENGTH = 64, GAE_SGNS_MAX_DIM = 128,
       GAE_SGNS_MAX_NEGATIVES = 1024, GAE_SGNS_SCALE_BITS = 32 };
enum { GAE_DEEPWALK_ERR_COLUMN = 1, GAE_DEEPWALK_ERR_INDPTR = 2, GAE_DEEPWALK_ERR_START = 4, GAE_DEEPWALK_ERR_RANGE = 8,
       GAE_DEEPWALK_ERR_NODE = 16, GAE_DEEPWALK_ERR_ORDER = 32, GAE_DEEPWALK_ERR_NONFINITE = 64 };
#define GAE_DEEPWALK_WALK_DRAW 0x3700000000ull
#define GAE_SGNS_NEG_DRAW 0x3800000000ull
#define GAE_SGNS_INIT_DRAW 0x3900000000ull

int gae_random_walks(const int64_t *indptr, const int32_t *indices, int64_t n, int64_t nnz, const int32_t *starts, int64_t m,
                     int64_t walks_per_start, int64_t length, uint64_t seed, int32_t *walks, int64_t *status, void *stream);

int gae_sgns_init(float *W, int64_t n, int64_t d, uint64_t seed, float bound, void *stream);

int gae_sgns_walk_order(int64_t n_walks, uint64_t seed, int64_t epoch, int32_t *order, void *stream);

int gae_sgns_accumulate(const int32_t *walks, int64_t n_walks, int64_t length, const int32_t *order, int64_t first,
                        int64_t count, const int64_t *cum, int64_t n, int64_t d, int64_t window, int64_t negatives,
                        int64_t shared_negatives, uint64_t seed, int64_t epoch, const float *W, const float *C, int64_t *AW,
                        int64_t *AC, int64_t *status, void *stream);

int gae_sgns_update(float *W, float *C, float *HW, float *HC, int64_t *AW, int64_t *AC, int64_t n, int64_t d, float lr,
                    float eps, int64_t *status, void *stream);

int gae_x_decoder_bce_defer_finalize(gae_bce_tail *tail_out);

int gae_x_decoder_bce_finalize(const gae_bce_tail *tail, void *stream);

/* (from gae_hip.h: K12: Adam) */
/* ... plus the deferred final reduction of the step's loss (gae_x_decoder_bce_defer_finalize; tail may be NULL) as one
 * more block of the same launch: one kernel node fewer in a captured training step. */
int gae_x_adam_step_tail(const gae_adam_tensor *tensors_host, int32_t n_tensors, float lr, float beta1, float beta2,
                       float eps, float weight_decay, uint64_t *state_dev, const gae_bce_tail *tail, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GAE_HIP_EXPERIMENTAL_H */
