// The walk of the molecule-set kernels: K19 gae_embed_graphs and K20 gae_score_graphs (embed.hip), K21
// gae_embed_graphs_bwd (embed_bwd.hip).  What the three have in common lives here, once: K21 runs K19's forward again
// and its ReLU pass masks depend on reproducing K19's bits, so the pieces below are the same code, not copies that
// agree.  Each kernel keeps its own loop (issue -> the group's turn -> the layers -> its tail) and calls these.
//
// Layout.  A wave owns S <= 64 consecutive output slots; lane t loads slot t's graph id and node range ONCE
// (load_slot).  The wave then walks its slots in groups: as many consecutive graphs as fit 64 rows (pack_group: a
// register prefix scan, no memory), one atom per lane.  LDS buffers private to the wave hold the activations
// [64 rows][width] of the layer being read and the one being written; the weights of all layers are staged once per
// block, transposed and zero padded to [f_in][JP] (stage_layer; JP = output width rounded up to 8).
//   aggregate   lane r walks its CSR row (the first 4 column ids sit in registers, longer rows continue from the CSR)
//               and adds the LDS rows of its neighbours in CSR order, four features at a time; the sums go to the
//               lane's own row of the buffer being written
//   transform   y_j = act(b_j + sum_k m_k W_jk), k ascending over the true input width: JP accumulators per lane, per k
//               one read of m_k and JP / 4 broadcast reads of row k of W^T (every lane reads the same address).  The
//               sums are fp32 fmaf chains -- the arithmetic v_mfma_f32_32x32x2_f32 performs, at the same peak rate: on
//               gfx950 the fp32 MFMA shares the fp32 FMA lanes with the VALU (common.h), so atoms-as-lanes costs no
//               throughput, needs no operand shuffles between the layers and fills 64 rows instead of 32
//               (transform_keep<JP>; each kernel switches on JP itself)
// Every output element is its own chain over the graph's own rows, so a graph's rows have the same bits at any position,
// in any group, in any launch, in any of the three kernels.
//
// Loads.  The row bounds of the NEXT group and its uint8 feature row (3 x 16 bytes for 39 features) are issued into
// registers by the kernel right after pack_group, before the current group's layers run, and written to LDS only when
// that group's turn comes (lane_turn, unpack_u8_row).  fp32 feature rows are 16 vectors: K19 and K20 prefetch them the
// same way, K21 loads them at the group's turn, four at a time (prefetching spilled there: DESIGN.md K21).
//
// Safety.  A graph id outside [0, G), a node range outside [0, N] or above the caller's row bound (64, or K20's
// max_graph_nodes) makes a slot that no group takes: the kernel refuses it (a row of NaN, invalid scores, no
// contribution to a gradient).  A row pointer outside [0, E] reads as an empty row; a column id outside the graph's
// own rows is skipped: nothing outside the arrays is read or written.
//
// The host side below is what the three entry points ask of their common arguments (Request), with one set of
// messages, and the launch with more than 48 KB of dynamic LDS.
#pragma once
#include "common.h"

namespace gae {
namespace walk {

constexpr int kMaxLayers = 4;
constexpr int kMaxWidth = 64;
constexpr int kRows = 64;         // rows of a group: one atom per lane
constexpr int kRegNb = 4;         // column ids of a row kept in registers

// LDS written by one lane of a wave and read by another: LDS operations of a wave complete in order, the fence keeps
// the compiler from moving them
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

struct Lane {                     // one atom of the current group
    bool active;
    int mb, mn;                   // first row and node count of its graph in the group
    int g0;                       // first global row of its graph
    int e0, e1;
    int nb[kRegNb];               // group rows of its first neighbours, -1 = none
    float sc;
};

// one layer's W^T zero padded to [fi][jp] into `wt` and its bias (zeros without one) into `bl`, by all threads of the block
__device__ __forceinline__ void stage_layer(const float *W, int64_t ldw, const float *bias, int fi, int fo, int jp,
                                            float *wt, float *bl, int tid, int nthreads)
{
#pragma unroll 4
    for (int idx = tid; idx < fi * jp; idx += nthreads) {
        const int k = idx / jp, j = idx - k * jp;
        const float v = W[j < fo ? j * ldw + k : 0];
        wt[idx] = j < fo ? v : 0.f;
    }
    for (int j = tid; j < jp; j += nthreads) bl[j] = (bias && j < fo) ? bias[j] : 0.f;
}

// this wave's slots: lane t < avail holds slot k0 + t (graph id -> node range).  A slot that cannot be taken (bad id,
// bad range, more than max_rows rows) gets sn = kRows + 1: it never fits a group
template <class Args>
__device__ __forceinline__ void load_slot(const Args &a, int64_t k0, int lane, int avail, int max_rows, int &sn,
                                          int &sr0)
{
    const bool sv = lane < avail;
    const int64_t gid = sv ? (a.graph_ids ? a.graph_ids[k0 + lane] : k0 + lane) : -1;
    bool ok = sv && gid >= 0 && gid < a.G;
    int64_t r0 = 0, r1 = 0;
    if (ok) { r0 = a.graph_ptr[gid]; r1 = a.graph_ptr[gid + 1]; }
    ok = ok && r0 >= 0 && r1 >= r0 && r1 <= a.N && r1 - r0 <= max_rows;
    sn = ok ? int(r1 - r0) : kRows + 1;
    sr0 = ok ? int(r0) : 0;
}

// the group that starts at slot `at`: the cnt consecutive slots whose rows fit 64 (0: slot `at` cannot be taken), the
// first group row of the lane's OWN slot (gbase), the lane's atom without its row bounds (the kernel loads e0 / e1 with
// the feature row); returns the rows of the group
__device__ __forceinline__ int pack_group(int at, int lane, int avail, int sn, int sr0, int &cnt, int &gbase, Lane &ln)
{
    int v = (lane >= at && lane < avail) ? sn : 0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    const bool take = lane >= at && lane < avail && v <= kRows;
    cnt = __builtin_popcountll(__ballot(take));
    const int rows = cnt ? __shfl(v, at + cnt - 1, 64) : 0;
    gbase = v - sn;
    ln.active = lane < rows;
    ln.mb = 0; ln.mn = 0; ln.g0 = 0; ln.e0 = 0; ln.e1 = 0; ln.sc = 0.f;
    for (int m = at; m < at + cnt; ++m) {
        const int b = __shfl(gbase, m, 64), n = __shfl(sn, m, 64), g0 = __shfl(sr0, m, 64);
        if (lane >= b && lane < b + n) { ln.mb = b; ln.mn = n; ln.g0 = g0; }
    }
    return rows;
}

// the lane's atom at its group's turn: row bounds outside [0, E] read as an empty row, the first kRegNb neighbours as
// group rows (a column outside the graph's own rows: none), 1 / sqrt(in-degree)
__device__ __forceinline__ void lane_turn(const int32_t *indices, int64_t E, Lane &me)
{
    const bool rowok = me.active && me.e0 >= 0 && me.e1 >= me.e0 && int64_t(me.e1) <= E;
    if (!rowok) me.e0 = me.e1 = 0;
#pragma unroll
    for (int q = 0; q < kRegNb; ++q) {
        me.nb[q] = -1;
        if (me.e0 + q < me.e1) {
            const int c = indices[me.e0 + q] - me.g0;
            if (c >= 0 && c < me.mn) me.nb[q] = me.mb + c;
        }
    }
    const int deg = me.e1 - me.e0;
    me.sc = deg > 0 ? 1.0f / sqrtf(float(deg)) : 0.f;
}

// a uint8 feature row held as raw 16-byte vectors x[0 .. 3] -> f0 floats (zeros up to the next multiple of 4) at dst
__device__ __forceinline__ void unpack_u8_row(const v4f *x, int f0, v4f *dst)
{
#pragma unroll
    for (int c = 0; c < 16; ++c)
        if (4 * c < f0) {
            const unsigned w = __float_as_uint(x[c / 4][c & 3]);
            v4f v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = 4 * c + i < f0 ? float((w >> (8 * i)) & 0xffu) : 0.f;
            dst[c] = v;
        }
}

// M = (D^-1/2) A (D^-1/2) H of the lane's row, four features per trip, into its own row of `out`
template <class Args>
__device__ __forceinline__ void aggregate(const Args &a, const Lane &ln, int row, int fi, const float *in, int sin,
                                          float *out, int sout, const float *scale)
{
    float s[kRegNb];
#pragma unroll
    for (int q = 0; q < kRegNb; ++q) s[q] = (a.norm_both && ln.nb[q] >= 0) ? scale[ln.nb[q]] : 1.f;
    const bool tail = ln.e1 - ln.e0 > kRegNb;
    for (int c = 0; c < (fi + 3) / 4; ++c) {
        v4f m = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < kRegNb; ++q)
            if (ln.nb[q] >= 0) {
                const v4f v = *reinterpret_cast<const v4f *>(in + ln.nb[q] * sin + 4 * c);
                if (a.norm_both) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) m[i] = fmaf(s[q], v[i], m[i]);
                } else {
                    m += v;
                }
            }
        if (tail)
            for (int e = ln.e0 + kRegNb; e < ln.e1; ++e) {      // the rare long row continues from the CSR
                const int u = a.indices[e] - ln.g0;
                if (u >= 0 && u < ln.mn) {
                    const v4f v = *reinterpret_cast<const v4f *>(in + (ln.mb + u) * sin + 4 * c);
                    if (a.norm_both) {
                        const float su = scale[ln.mb + u];
#pragma unroll
                        for (int i = 0; i < 4; ++i) m[i] = fmaf(su, v[i], m[i]);
                    } else {
                        m += v;
                    }
                }
            }
        if (a.norm_both) m *= ln.sc;
        *reinterpret_cast<v4f *>(out + row * sout + 4 * c) = m;
    }
}

// y = act(M W^T + b) of the lane's row: M is read from `mrow`, y written to `yrow` (which may be mrow: K19 and K20
// replace M); returns the pass mask (bit j: output j went through the activation unchanged), which K21 keeps
template <int JP>
__device__ __forceinline__ uint64_t transform_keep(const float *Wt, const float *bl, int fi, bool relu, const float *mrow,
                                                   float *yrow)
{
    float y[JP];
#pragma unroll
    for (int j = 0; j < JP; ++j) y[j] = 0.f;
#pragma unroll 1
    for (int k = 0; k < fi; ++k) {
        const float mk = mrow[k];
        const v4f *w = reinterpret_cast<const v4f *>(Wt + k * JP);
#pragma unroll
        for (int q = 0; q < JP / 4; ++q) {
            const v4f wv = w[q];
#pragma unroll
            for (int i = 0; i < 4; ++i) y[4 * q + i] = fmaf(mk, wv[i], y[4 * q + i]);
        }
    }
    uint64_t mask = 0;
#pragma unroll
    for (int q = 0; q < JP / 4; ++q) {
        const v4f b = *reinterpret_cast<const v4f *>(bl + 4 * q);
        v4f v;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float t = y[4 * q + i] + b[i];
            const bool pass = !relu || t > 0.f || t != t;        // ReLU keeps a NaN
            v[i] = pass ? t : 0.f;
            mask |= uint64_t(pass) << (4 * q + i);
        }
        *reinterpret_cast<v4f *>(yrow + 4 * q) = v;
    }
    return mask;
}

// ---- host side ------------------------------------------------------------------------------------------------------
inline int round_up(int v, int q) { return (v + q - 1) / q * q; }

// the shapes the kernels take (K20 also the encoder of no layers, min_layers = 0: the feature rows are Z); `what` (may
// be NULL) receives the offending quantity
inline bool shape_taken(int64_t f_in, int64_t n_layers, const int64_t *widths, int64_t max_graph_nodes, int min_layers,
                 char *what, size_t cap)
{
    if (n_layers < min_layers || n_layers > kMaxLayers) {
        if (what) snprintf(what, cap, "n_layers = %lld outside %d..%d", (long long)n_layers, min_layers, kMaxLayers);
        return false;
    }
    if (f_in < 1 || f_in > kMaxWidth) {
        if (what) snprintf(what, cap, "input width f_in = %lld outside 1..%d", (long long)f_in, kMaxWidth);
        return false;
    }
    for (int64_t l = 0; l < n_layers; ++l)
        if (widths[l] < 1 || widths[l] > kMaxWidth) {
            if (what)
                snprintf(what, cap, "width of layer %lld = %lld outside 1..%d", (long long)l, (long long)widths[l],
                         kMaxWidth);
            return false;
        }
    if (max_graph_nodes > kRows) {
        if (what)
            snprintf(what, cap, "max_graph_nodes = %lld above %d nodes per graph", (long long)max_graph_nodes, kRows);
        return false;
    }
    return true;
}

// what the three entry points ask of their common arguments, in this order; `fn` names the caller
struct Request {
    const int64_t *graph_ptr;
    int64_t n_graphs, n_nodes, n_edges, max_graph_nodes;
    const int32_t *indptr, *indices;
    const void *feat;
    int feat_dtype;
    int64_t ldf, f_in, n_layers;
    const int64_t *widths;
    const float *const *weights;
    const int64_t *ldw;
    const float *const *biases;
    const int *acts;
    int norm;
    const int64_t *graph_ids;
    int64_t n_out;
};

inline int check_layers(const char *fn, const Request &r, int min_layers)
{
    GAE_REQUIRE((min_layers == 0 && r.n_layers == 0) || (r.widths && r.weights && r.ldw && r.acts), GAE_E_NULL,
                "%s: widths / weights / ldw / acts is NULL", fn);
    GAE_REQUIRE(r.n_graphs >= 0 && r.n_nodes >= 0 && r.n_edges >= 0 && r.n_out >= 0 && r.max_graph_nodes >= 0, GAE_E_SIZE,
                "%s: negative n_graphs = %lld, n_nodes = %lld, n_edges = %lld, n_out = %lld or "
                "max_graph_nodes = %lld", fn, (long long)r.n_graphs, (long long)r.n_nodes, (long long)r.n_edges,
                (long long)r.n_out, (long long)r.max_graph_nodes);
    GAE_REQUIRE(r.n_nodes < (int64_t(1) << 31) && r.n_edges < (int64_t(1) << 31), GAE_E_SIZE,
                "%s: n_nodes = %lld or n_edges = %lld beyond the int32 CSR", fn, (long long)r.n_nodes,
                (long long)r.n_edges);
    char what[160];
    GAE_REQUIRE(shape_taken(r.f_in, r.n_layers, r.widths, r.max_graph_nodes, min_layers, what, sizeof what), GAE_E_RANGE,
                "%s: %s", fn, what);
    GAE_REQUIRE(r.norm == GAE_EMBED_NORM_NONE || r.norm == GAE_EMBED_NORM_BOTH, GAE_E_RANGE,
                "%s: unknown norm code %d (0 = none, 1 = both)", fn, r.norm);
    GAE_REQUIRE(r.feat_dtype == GAE_F32 || r.feat_dtype == GAE_U8, GAE_E_DTYPE,
                "%s: feature dtype %d (GAE_F32 or GAE_U8)", fn, r.feat_dtype);
    for (int64_t l = 0; l < r.n_layers; ++l) {
        GAE_REQUIRE(r.acts[l] == GAE_ACT_IDENTITY || r.acts[l] == GAE_ACT_RELU, GAE_E_DTYPE,
                    "%s: unknown activation code %d of layer %lld", fn, r.acts[l], (long long)l);
        GAE_REQUIRE(r.weights[l], GAE_E_NULL, "%s: the weight of layer %lld is NULL", fn, (long long)l);
        GAE_REQUIRE(r.ldw[l] >= (l ? r.widths[l - 1] : r.f_in), GAE_E_SIZE,
                    "%s: leading dimension ldw = %lld of layer %lld below its input width", fn,
                    (long long)r.ldw[l], (long long)l);
    }
    return GAE_OK;
}

inline int check_feature_rows(const char *fn, const Request &r)
{
    const int64_t row_elems = r.feat_dtype == GAE_U8 ? (r.f_in + 15) / 16 * 16 : (r.f_in + 3) / 4 * 4;
    GAE_REQUIRE(r.ldf >= row_elems, GAE_E_SIZE,
                "%s: feature rows of ldf = %lld elements, %lld needed (whole 16-byte vectors)", fn,
                (long long)r.ldf, (long long)row_elems);
    return GAE_OK;
}

inline int check_arrays(const char *fn, const Request &r)
{
    GAE_REQUIRE(r.n_nodes == 0 || (r.indptr && r.feat), GAE_E_NULL, "%s: indptr / feat is NULL", fn);
    GAE_REQUIRE(r.n_edges == 0 || r.indices, GAE_E_NULL, "%s: indices is NULL", fn);
    const int64_t row_bytes = r.ldf * (r.feat_dtype == GAE_U8 ? 1 : 4);
    GAE_REQUIRE(r.n_nodes == 0 || (gae::aligned16(r.feat) && row_bytes % 16 == 0), GAE_E_ALIGN,
                "%s: feature rows must start on 16-byte boundaries (pointer and ldf)", fn);
    return GAE_OK;
}

} // namespace walk
} // namespace gae
