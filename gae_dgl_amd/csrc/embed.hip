// K19: the molecule feature of a whole resident set in ONE launch (GAE.embed_graphs, ops.embed_graphs).
//
// For every selected member graph: the complete GCN encoder (gae.py:26-31,36-45: aggregate over in-edges, Linear + bias,
// ReLU on all but the last layer) on that graph's own rows, then the README readout [mean | sum | max] over its nodes.
// The node embeddings never go to HBM: inputs are read from the dataset as it is stored (uint8 or fp32 feature rows,
// the block-diagonal CSR with global column ids), 12 d bytes are written per graph.
//
// Layout.  A wave owns S <= 64 consecutive output slots; lane t loads slot t's graph id and node range ONCE.  The wave
// then walks its slots in groups: as many consecutive graphs as fit 64 rows (a register prefix scan, no memory), one
// atom per lane.  Two LDS buffers per wave hold the activations [64 rows][width] of the layer being read and the one
// being written; the weights of all layers are staged once per block, transposed and zero padded to [f_in][JP]
// (JP = output width rounded up to 8).
//   aggregate   lane r walks its CSR row (the first 4 column ids sit in registers, longer rows continue from the CSR)
//               and adds the LDS rows of its neighbours in CSR order, four features at a time; the sums go to the
//               lane's own row of the buffer being written
//   transform   y_j = act(b_j + sum_k m_k W_jk), k ascending over the true input width: JP accumulators per lane, per k
//               one read of m_k and JP / 4 broadcast reads of row k of W^T (every lane reads the same address).  The
//               sums are fp32 fmaf chains -- the arithmetic v_mfma_f32_32x32x2_f32 performs, at the same peak rate: on
//               gfx950 the fp32 MFMA shares the fp32 FMA lanes with the VALU (common.h), so atoms-as-lanes costs no
//               throughput, needs no operand shuffles between the layers and fills 64 rows instead of 32
//   readout     lane (slot, c) adds feature c of its graphs' rows first to last: an order that depends on the node count
//               alone
// Every output element is its own chain over the graph's own rows, so a graph's feature row has the same bits at any
// position, in any group, in any launch.  No atomics.
//
// Loads.  The feature row (3 x 16 bytes for 39 uint8 features) and the row bounds of the NEXT group are issued into
// registers before the current group's layers run, and written to LDS only when that group's turn comes.
//
// Safety.  A graph id outside [0, G), a node range outside [0, N] or above 64 rows gives a row of NaN; a row pointer
// outside [0, E] reads as an empty row; a column id outside the graph's own rows is skipped: nothing outside the arrays
// is read or written.
//
// Measured (tools/embed_bench.py, profiles/r10_embed_graphs.json; 39 -> 32 -> 16, uint8 features): the 249 455 molecules of
// the ZINC-sized set in 2.43 ms of kernel time (3.1 ms per call) against 15.5 ms for batch -> encode -> readout in chunks
// of 4096 and 389 ms in chunks of 128; 9 Tflop/s, 6 % of the fp32 peak -- LDS sets 1.5 waves per SIMD and feeds every
// FMA (DESIGN.md K19 lists the levers).  175 VGPRs, no scratch (uint8 form).
//
// K20: how well every selected member graph is reconstructed (GAE.score_graphs, ops.score_graphs).  The same walk and
// the same encoder -- graphs_body below is the body of both kernels, aggregate / transform are called by both -- with
// a second tail in place of the readout: the decoder on each graph's own ordered pairs, ranked and scored in LDS.
//   logits      lane r computes row r of its graph's n x n block: s_rb = the fmaf chain over k ascending, from 0.f, of
//               z_r[k] z_b[k] (Z rows from LDS, 16 bytes at a time), into the buffer the last layer no longer needs,
//               rows max_graph_nodes | 1 floats apart (odd: a column walk of a graph's lanes hits distinct banks)
//   labels      lane r walks its CSR row once more: a 64-bit mask of the columns that occur (a repeat counts once),
//               and S, the entries with repeats, for pos_weight
//   counting    lane r owns the positives of ITS row, in entry order: for the threshold t = s_rc it reads every pair
//               above the diagonal of its graph's block once (s_ab == s_ba bit for bit, so a hit counts twice; the
//               lanes of a graph read the same address: a broadcast) for all_ge / all_gt, and the pairs the masks mark
//               for pos_ge / pos_gt.  No cross-lane step per positive; the fp64 quotient pos_ge / all_ge is added in
//               the lane, neg_ge = all_ge - pos_ge and neg_gt are summed as integers
//   fold        lane m adds the rows of slot m first to last (tables in the buffer that held Z): integers, and the
//               fp64 sums of the AP terms and of the three loss sums (softplus(s) over all pairs; softplus(-s) and s
//               over the entries) in row order; wins = n_pos n_neg - sum neg_ge, ties = sum neg_ge - sum neg_gt
// Every number is a function of the graph's own rows in an order the graph alone fixes; integers are exact.  No atomics.
// The load of a lane is its row's positives times n (n - 1) / 2: a molecule's lanes are busy unevenly (2.2 bonds per
// atom on average, 4 at most), which is what the tail pays for needing no segmented reduction per positive.
//
// LDS (K20).  Per wave: the buffer that ends up holding Z (>= 64 x 16 floats: it takes the 896 floats of tables), the
// other buffer = the logit block, max(its K19 size, 64 x (max_graph_nodes | 1) floats), and K19's 192 floats of tables.
// 39 -> 32 -> 16 on ZINC (max 38 atoms): 64 x 39 = 2 496 floats fit the 64 x 44 the encoder needs anyway -- 53.8 KB per
// block as K19, 3 blocks = 6 waves per CU = 1.5 per SIMD, unchanged.  max_graph_nodes = 64 needs 64 x 65 floats: 64.6 KB
// per block for this model, 2 blocks = 1 wave per SIMD.  Registers: 227 VGPRs (uint8 form, 2 waves per SIMD), 270 (fp32
// form, 1 wave per SIMD, as K19's 261), no scratch.
#include "common.h"

namespace {

using gae::v4f;

constexpr int kMaxLayers = 4;
constexpr int kMaxWidth = 64;
constexpr int kRows = 64;         // rows of a group: one atom per lane
constexpr int kWaves = 2;         // waves per block
constexpr int kRegNb = 4;         // column ids of a row kept in registers

struct EmbedArgs {
    const int64_t *graph_ptr;
    const int32_t *indptr, *indices;
    const void *feat;
    int64_t ldf;                  // elements between feature rows
    int64_t G, N, E, B;
    int L;
    int width[kMaxLayers + 1];    // f_in, then every layer's output width
    int jp[kMaxLayers];           // outputs computed by layer l: its width rounded up to 8 (the pad outputs are zeros)
    int w_off[kMaxLayers], b_off[kMaxLayers];   // float offsets of the staged [f_in][jp] weights / [jp] bias
    const float *W[kMaxLayers];
    int64_t ldw[kMaxLayers];
    const float *bias[kMaxLayers];
    int act[kMaxLayers];
    int norm_both;
    const int64_t *graph_ids;
    float *out;
    int64_t ldo;
    int S;                        // output slots per wave
    int sa, sb;                   // row strides (floats) of the two activation buffers
    int wfloats;                  // floats of the staged weights and biases
    int wave_floats;              // floats of one wave's private LDS
};

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

// M = (D^-1/2) A (D^-1/2) H of the lane's row, four features per trip, into its own row of `out`
__device__ __forceinline__ void aggregate(const EmbedArgs &a, const Lane &ln, int row, int fi, const float *in, int sin,
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

// y = act(M W^T + b) of the lane's row: M is read from the lane's own row of `out`, y replaces it
template <int JP>
__device__ __forceinline__ void transform(const float *Wt, const float *bl, int fi, bool relu, float *mine)
{
    float y[JP];
#pragma unroll
    for (int j = 0; j < JP; ++j) y[j] = 0.f;
#pragma unroll 1
    for (int k = 0; k < fi; ++k) {
        const float mk = mine[k];
        const v4f *w = reinterpret_cast<const v4f *>(Wt + k * JP);
#pragma unroll
        for (int q = 0; q < JP / 4; ++q) {
            const v4f wv = w[q];
#pragma unroll
            for (int i = 0; i < 4; ++i) y[4 * q + i] = fmaf(mk, wv[i], y[4 * q + i]);
        }
    }
#pragma unroll
    for (int q = 0; q < JP / 4; ++q) {
        const v4f b = *reinterpret_cast<const v4f *>(bl + 4 * q);
        v4f v;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float t = y[4 * q + i] + b[i];
            v[i] = !relu || t > 0.f || t != t ? t : 0.f;         // ReLU keeps a NaN
        }
        *reinterpret_cast<v4f *>(mine + 4 * q) = v;
    }
}

// ---- K20: the decoder tail (see the header comment) ------------------------------------------------------------------
struct ScoreArgs {
    int64_t *counts;              // [B][4]: n_pos, n_neg, wins, ties
    double *ap;                   // [B]
    float *loss;                  // [B]
    int exclude_self;
    int max_nodes;                // the host's bound of a graph's rows: a larger graph is refused (the block is sized for it)
    int rs;                       // floats between two rows of the logit block: max_nodes | 1
    int z_in_b;                   // odd layer count: Z ends in buffer B, which then comes first
    int block_floats;             // floats of the second buffer = the logit block
};

// float offsets of the per-lane tables inside the buffer that held Z (dead once the logits are in the block)
enum { kTabLab = 0, kTabGe = 128, kTabGt = 192, kTabS = 256, kTabBad = 320, kTabAp = 384, kTabSp = 512, kTabA = 640,
       kTabB = 768, kTabFloats = 896 };

__device__ __forceinline__ void score_invalid(const ScoreArgs &t, int64_t k)
{
    int64_t *c = t.counts + 4 * k;
    c[0] = c[1] = c[2] = c[3] = -1;
    t.ap[k] = __builtin_nan("");
    t.loss[k] = __builtin_nanf("");
}

__device__ __forceinline__ float softplus(float x)
{
    return fmaxf(x, 0.f) + log1pf(__expf(-fabsf(x)));
}

// Z [64 rows][sz] of the group is final.  Lane r: its row of logits into the block, its label mask from its CSR row,
// then for each positive of its row (entry order, first occurrence) the counts over all pairs of its graph.
__device__ __forceinline__ void score_tail(const EmbedArgs &a, const ScoreArgs &t, const Lane &me, int lane, int d,
                                           float *Z, int sz, float *blk, const int *mbase, const int *mcount, int ccnt,
                                           int64_t slot0)
{
    const int RS = t.rs, n = me.mn, mb = me.mb, li = lane - mb;
    float *myrow = blk + lane * RS;
    // ---- logits of the lane's row against the rows of its own graph: fmaf chains from 0.f, k ascending
    double sp = 0.0;
    bool bad = false;
    if (me.active) {
        const float *zi = Z + lane * sz;
        const int d4 = d & ~3;
        for (int b = 0; b < n; ++b) {
            const float *zb = Z + (mb + b) * sz;
            float s = 0.f;
            for (int k = 0; k < d4; k += 4) {
                const v4f x = *reinterpret_cast<const v4f *>(zi + k), y = *reinterpret_cast<const v4f *>(zb + k);
#pragma unroll
                for (int i = 0; i < 4; ++i) s = fmaf(x[i], y[i], s);
            }
            for (int k = d4; k < d; ++k) s = fmaf(zi[k], zb[k], s);
            myrow[b] = s;
            bad = bad || !(fabsf(s) < INFINITY);
            sp += double(softplus(s));               // the loss sees all n^2 ordered pairs, self pairs included
        }
    }
    wave_sync();                                     // Z is dead from here on: its buffer holds the tables
    // ---- label mask of the lane's row: bit c = column g0 + c occurs in it; S counts the entries with repeats
    uint64_t *tlab = reinterpret_cast<uint64_t *>(Z + kTabLab);
    uint64_t lab = 0;
    unsigned S = 0;
    if (me.active) {
        for (int e = me.e0; e < me.e1; ++e) {
            const int c = a.indices[e] - me.g0;
            if (c >= 0 && c < n) { lab |= 1ull << c; ++S; }
        }
        if (t.exclude_self) lab &= ~(1ull << li);
    }
    tlab[lane] = lab;
    wave_sync();
    // ---- the lane's positives, in CSR order.  all = ordered pairs of the graph (s_rb == s_br bit for bit: the pairs
    // above the diagonal are read once and count twice), pos = the pairs the masks mark
    unsigned sge = 0, sgt = 0;                       // sums over the lane's positives of neg_ge, neg_gt (<= 64 * 4096)
    double ap = 0.0, la = 0.0, lb = 0.0;
    if (me.active) {
        uint64_t seen = 0;
        for (int e = me.e0; e < me.e1; ++e) {
            const int c = a.indices[e] - me.g0;
            if (c < 0 || c >= n) continue;
            const float x = myrow[c];
            la += double(softplus(-x));              // y_ij counts every entry, repeats and self loops included
            lb += double(x);
            const uint64_t bit = 1ull << c;
            if (!(lab & bit) || (seen & bit)) continue;
            seen |= bit;
            unsigned ge = 0, gt = 0;
            for (int r = 0; r < n; ++r) {
                const float *ra = blk + (mb + r) * RS;
                for (int b = r + 1; b < n; ++b) {
                    const float s = ra[b];
                    ge += s >= x;
                    gt += s > x;
                }
            }
            ge *= 2; gt *= 2;
            if (!t.exclude_self)
                for (int r = 0; r < n; ++r) {
                    const float s = blk[(mb + r) * RS + r];
                    ge += s >= x;
                    gt += s > x;
                }
            unsigned pge = 0, pgt = 0;
            for (int r = 0; r < n; ++r) {
                const float *ra = blk + (mb + r) * RS;
                uint64_t m = tlab[mb + r];
                while (m) {
                    const int b = __builtin_ctzll(m);
                    m &= m - 1;
                    const float s = ra[b];
                    pge += s >= x;
                    pgt += s > x;
                }
            }
            ap += double(pge) / double(ge);
            sge += ge - pge;
            sgt += gt - pgt;
        }
    }
    reinterpret_cast<unsigned *>(Z + kTabGe)[lane] = sge;
    reinterpret_cast<unsigned *>(Z + kTabGt)[lane] = sgt;
    reinterpret_cast<unsigned *>(Z + kTabS)[lane] = S;
    reinterpret_cast<unsigned *>(Z + kTabBad)[lane] = bad ? 1u : 0u;
    reinterpret_cast<double *>(Z + kTabAp)[lane] = ap;
    reinterpret_cast<double *>(Z + kTabSp)[lane] = sp;
    reinterpret_cast<double *>(Z + kTabA)[lane] = la;
    reinterpret_cast<double *>(Z + kTabB)[lane] = lb;
    wave_sync();
    // ---- lane m folds the rows of slot m first to last: integers, and fp64 sums in row order
    if (lane < ccnt) {
        const int b0 = mbase[lane], gn = mcount[lane];
        int64_t n_pos = 0, tge = 0, tgt = 0, tS = 0;
        unsigned anybad = 0;
        double tap = 0.0, tsp = 0.0, ta = 0.0, tb = 0.0;
        for (int r = b0; r < b0 + gn; ++r) {
            n_pos += __builtin_popcountll(tlab[r]);
            tge += reinterpret_cast<const unsigned *>(Z + kTabGe)[r];
            tgt += reinterpret_cast<const unsigned *>(Z + kTabGt)[r];
            tS += reinterpret_cast<const unsigned *>(Z + kTabS)[r];
            anybad |= reinterpret_cast<const unsigned *>(Z + kTabBad)[r];
            tap += reinterpret_cast<const double *>(Z + kTabAp)[r];
            tsp += reinterpret_cast<const double *>(Z + kTabSp)[r];
            ta += reinterpret_cast<const double *>(Z + kTabA)[r];
            tb += reinterpret_cast<const double *>(Z + kTabB)[r];
        }
        const int64_t k = slot0 + lane;
        if (anybad) {
            score_invalid(t, k);
        } else {
            const int64_t nn = int64_t(gn) * gn, n_neg = nn - (t.exclude_self ? gn : 0) - n_pos;
            int64_t *c = t.counts + 4 * k;
            c[0] = n_pos;
            c[1] = n_neg;
            c[2] = n_pos * n_neg - tge;              // wins = sum_p (n_neg - neg_ge(p))
            c[3] = tge - tgt;                        // ties = sum_p (neg_ge(p) - neg_gt(p))
            t.ap[k] = n_pos > 0 && n_neg > 0 ? tap / double(n_pos) : __builtin_nan("");
            float l = __builtin_nanf("");
            if (n_pos > 0) {
                const double pw = (double(nn) - double(tS)) / double(tS);      // train_inductive.py:46
                l = float((tsp + (pw - 1.0) * ta - tb) / double(nn));
            }
            t.loss[k] = l;
        }
    }
}

// The walk both kernels share: the slots of a wave, their groups, the encoder of a group in LDS.  SCORE = false ends a
// group with K19's readout, SCORE = true with K20's decoder tail (score_tail).
template <bool U8, bool SCORE>
__device__ __forceinline__ void graphs_body(const EmbedArgs &a, const ScoreArgs &t)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- the weights of all layers, once per block: W^T zero padded to [f_in][jp]
    for (int l = 0; l < a.L; ++l) {
        const int jp = a.jp[l], fi = a.width[l], fo = a.width[l + 1];
        const float *W = a.W[l];
        const int64_t ldw = a.ldw[l];
        float *dst = lds + a.w_off[l];
#pragma unroll 4
        for (int idx = tid; idx < fi * jp; idx += kWaves * 64) {
            const int k = idx / jp, j = idx - k * jp;
            const float v = W[j < fo ? j * ldw + k : 0];
            dst[idx] = j < fo ? v : 0.f;
        }
        const float *bias = a.bias[l];
        for (int j = tid; j < jp; j += kWaves * 64) lds[a.b_off[l] + j] = (bias && j < fo) ? bias[j] : 0.f;
    }
    __syncthreads();

    float *bufA = lds + a.wfloats + wave * a.wave_floats;
    float *bufB = bufA + kRows * a.sa;
    float *scale = bufB + kRows * a.sb;
    if constexpr (SCORE) {
        // the buffer that ends up holding Z comes first; the other one is the logit block and may be longer
        float *base = bufA;
        bufA = base + (t.z_in_b ? kRows * a.sb : 0);
        bufB = base + (t.z_in_b ? 0 : kRows * a.sa);
        scale = base + kRows * (t.z_in_b ? a.sb : a.sa) + t.block_floats;
    }
    int *mbase = reinterpret_cast<int *>(scale + kRows);
    int *mcount = mbase + kRows;

    const int64_t k0 = (int64_t(blockIdx.x) * kWaves + wave) * a.S;
    if (k0 >= a.B) return;
    const int avail = int(a.B - k0 < a.S ? a.B - k0 : a.S);
    const int d = a.width[a.L];
    const int f0 = a.width[0];

    // ---- this wave's slots: lane t holds slot t (graph id -> node range), loaded once
    int sn = 0, sr0 = 0;
    {
        const bool sv = lane < avail;
        const int64_t gid = sv ? (a.graph_ids ? a.graph_ids[k0 + lane] : k0 + lane) : -1;
        bool ok = sv && gid >= 0 && gid < a.G;
        int64_t r0 = 0, r1 = 0;
        if (ok) { r0 = a.graph_ptr[gid]; r1 = a.graph_ptr[gid + 1]; }
        ok = ok && r0 >= 0 && r1 >= r0 && r1 <= a.N && r1 - r0 <= kRows;
        if constexpr (SCORE) ok = ok && r1 - r0 <= t.max_nodes;      // the logit block is sized for max_graph_nodes
        sn = ok ? int(r1 - r0) : kRows + 1;        // a slot that cannot be taken never fits a group
        sr0 = ok ? int(r0) : 0;
    }

    // ---- the group that starts at slot `pos` and the loads issued for it
    constexpr int NX = U8 ? 4 : 16;                // 16-byte vectors of a feature row held in registers
    const int nvec = U8 ? (f0 + 15) / 16 : (f0 + 3) / 4;
    int pos = 0, cnt = 0, gbase = 0;
    Lane ln;
    v4f x[NX];

    auto issue = [&](int at) {
        pos = at;
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
        if (ln.active) {
            const int64_t gr = int64_t(ln.g0) + (lane - ln.mb);
            ln.e0 = a.indptr[gr];
            ln.e1 = a.indptr[gr + 1];
            const v4f *row = reinterpret_cast<const v4f *>(static_cast<const char *>(a.feat) + gr * a.ldf * (U8 ? 1 : 4));
#pragma unroll
            for (int q = 0; q < NX; ++q)
                if (q < nvec) x[q] = row[q];
        }
    };

    issue(0);
    while (pos < avail) {
        if (cnt == 0) {
            // a slot that cannot be taken (bad id, bad range, above 64 rows): a row of NaN
            if constexpr (SCORE) {
                if (lane == 0) score_invalid(t, k0 + pos);
            } else {
                float *o = a.out + (k0 + pos) * a.ldo;
                for (int c = lane; c < 3 * d; c += 64) o[c] = __builtin_nanf("");
            }
            issue(pos + 1);
            continue;
        }
        // ---- the group's turn: its registers go to LDS
        const Lane cur = ln;
        const int cpos = pos, ccnt = cnt;
        Lane me = cur;
        {
            const int mi = lane - cpos;
            if (mi >= 0 && mi < ccnt) { mbase[mi] = gbase; mcount[mi] = sn; }
            const bool rowok = me.active && me.e0 >= 0 && me.e1 >= me.e0 && int64_t(me.e1) <= a.E;
            if (!rowok) me.e0 = me.e1 = 0;
#pragma unroll
            for (int q = 0; q < kRegNb; ++q) {
                me.nb[q] = -1;
                if (me.e0 + q < me.e1) {
                    const int c = a.indices[me.e0 + q] - me.g0;
                    if (c >= 0 && c < me.mn) me.nb[q] = me.mb + c;
                }
            }
            const int deg = me.e1 - me.e0;
            me.sc = deg > 0 ? 1.0f / sqrtf(float(deg)) : 0.f;
            scale[lane] = me.sc;
            if (me.active) {
                v4f *dst = reinterpret_cast<v4f *>(bufA + lane * a.sa);
                if (U8) {
#pragma unroll
                    for (int c = 0; c < 16; ++c)
                        if (4 * c < f0) {
                            const unsigned w = __float_as_uint(x[c / 4][c & 3]);
                            v4f v;
#pragma unroll
                            for (int i = 0; i < 4; ++i) v[i] = 4 * c + i < f0 ? float((w >> (8 * i)) & 0xffu) : 0.f;
                            dst[c] = v;
                        }
                } else {
#pragma unroll
                    for (int c = 0; c < 16; ++c)
                        if (4 * c < f0) {
                            v4f v = x[c];
#pragma unroll
                            for (int i = 0; i < 4; ++i) v[i] = 4 * c + i < f0 ? v[i] : 0.f;    // pad columns are not data
                            dst[c] = v;
                        }
                }
            }
            wave_sync();
        }
        issue(cpos + ccnt);                          // the next group's loads are in flight while the layers run
        const float *in = bufA;
        float *out = bufB;
        int sin = a.sa, sout = a.sb;
        for (int l = 0; l < a.L; ++l) {
            if (me.active) {
                const int fi = a.width[l];
                aggregate(a, me, lane, fi, in, sin, out, sout, scale);
                const float *Wt = lds + a.w_off[l], *bl = lds + a.b_off[l];
                const bool relu = a.act[l] == GAE_ACT_RELU;
                float *mine = out + lane * sout;
                switch (a.jp[l]) {
                case 8: transform<8>(Wt, bl, fi, relu, mine); break;
                case 16: transform<16>(Wt, bl, fi, relu, mine); break;
                case 24: transform<24>(Wt, bl, fi, relu, mine); break;
                case 32: transform<32>(Wt, bl, fi, relu, mine); break;
                case 40: transform<40>(Wt, bl, fi, relu, mine); break;
                case 48: transform<48>(Wt, bl, fi, relu, mine); break;
                case 56: transform<56>(Wt, bl, fi, relu, mine); break;
                default: transform<64>(Wt, bl, fi, relu, mine); break;
                }
            }
            wave_sync();
            const float *t = in; in = out; out = const_cast<float *>(t);
            const int ts = sin; sin = sout; sout = ts;
        }
        // ---- readout: Z = `in` now; lane (slot, c) walks the rows of its graphs first to last
        if constexpr (SCORE) {
            score_tail(a, t, me, lane, d, const_cast<float *>(in), sin, out, mbase, mcount, ccnt, k0 + cpos);
        } else {
            int DP = 1;
            while (DP < d) DP <<= 1;
            const int c = lane & (DP - 1), slot = lane / DP, RS = 64 / DP;
            if (c < d) {
                for (int m = slot; m < ccnt; m += RS) {
                    const int b = mbase[m], n = mcount[m];
                    float s = 0.f, mx = -INFINITY;
                    for (int r = b; r < b + n; ++r) {
                        const float v = in[r * sin + c];
                        s += v;
                        mx = fmaxf(mx, v);
                    }
                    float *o = a.out + (k0 + cpos + m) * a.ldo;
                    o[c] = n > 0 ? s / float(n) : 0.f;
                    o[d + c] = s;
                    o[2 * d + c] = n > 0 ? mx : 0.f;
                }
            }
        }
        wave_sync();                                 // the next group's turn overwrites the tables and buffer A
    }
}

template <bool U8>
__global__ __launch_bounds__(kWaves * 64) void embed_graphs_kernel(const EmbedArgs a)
{
    graphs_body<U8, false>(a, ScoreArgs{});
}

template <bool U8>
__global__ __launch_bounds__(kWaves * 64) void score_graphs_kernel(const EmbedArgs a, const ScoreArgs t)
{
    graphs_body<U8, true>(a, t);
}

int round_up(int v, int q) { return (v + q - 1) / q * q; }

// the shapes the kernels take (K20 also the encoder of no layers: the feature rows are Z); `what` (may be NULL)
// receives the offending quantity
bool shape_taken(int64_t f_in, int64_t n_layers, const int64_t *widths, int64_t max_graph_nodes, int min_layers,
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

// what gae_embed_graphs and gae_score_graphs ask of their common arguments, in this order; `fn` names the caller
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

int check_layers(const char *fn, const Request &r, int min_layers)
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

int check_feature_rows(const char *fn, const Request &r)
{
    const int64_t row_elems = r.feat_dtype == GAE_U8 ? (r.f_in + 15) / 16 * 16 : (r.f_in + 3) / 4 * 4;
    GAE_REQUIRE(r.ldf >= row_elems, GAE_E_SIZE,
                "%s: feature rows of ldf = %lld elements, %lld needed (whole 16-byte vectors)", fn,
                (long long)r.ldf, (long long)row_elems);
    return GAE_OK;
}

int check_arrays(const char *fn, const Request &r)
{
    GAE_REQUIRE(r.n_nodes == 0 || (r.indptr && r.feat), GAE_E_NULL, "%s: indptr / feat is NULL", fn);
    GAE_REQUIRE(r.n_edges == 0 || r.indices, GAE_E_NULL, "%s: indices is NULL", fn);
    const int64_t row_bytes = r.ldf * (r.feat_dtype == GAE_U8 ? 1 : 4);
    GAE_REQUIRE(r.n_nodes == 0 || (gae::aligned16(r.feat) && row_bytes % 16 == 0), GAE_E_ALIGN,
                "%s: feature rows must start on 16-byte boundaries (pointer and ldf)", fn);
    return GAE_OK;
}

// the kernel arguments of a checked request: staged weights, row strides of the two buffers, slots per wave.  The LDS
// of a wave (wave_floats) is K19's; gae_score_graphs replaces it.
int64_t fill_args(const Request &r, EmbedArgs &a)
{
    a.graph_ptr = r.graph_ptr; a.indptr = r.indptr; a.indices = r.indices; a.feat = r.feat; a.ldf = r.ldf;
    a.G = r.n_graphs; a.N = r.n_nodes; a.E = r.n_edges; a.B = r.n_out;
    a.L = int(r.n_layers);
    a.width[0] = int(r.f_in);
    for (int l = 0; l < a.L; ++l) a.width[l + 1] = int(r.widths[l]);
    for (int l = a.L + 1; l <= kMaxLayers; ++l) a.width[l] = 0;
    int off = 0;
    for (int l = 0; l < kMaxLayers; ++l) {
        a.jp[l] = a.w_off[l] = a.b_off[l] = a.act[l] = 0;
        a.W[l] = nullptr; a.bias[l] = nullptr; a.ldw[l] = 0;
    }
    int sa = round_up(a.width[0], 4), sb = 0;      // (no layers: buffer A holds the feature rows and nothing else)
    for (int l = 0; l < a.L; ++l) {
        const int fq = round_up(a.width[l], 4);    // the input (and its aggregate) in whole 16-byte vectors
        a.jp[l] = round_up(a.width[l + 1], 8);
        a.w_off[l] = off; off += a.width[l] * a.jp[l];
        a.b_off[l] = off; off += a.jp[l];
        a.W[l] = r.weights[l]; a.ldw[l] = r.ldw[l]; a.bias[l] = r.biases ? r.biases[l] : nullptr; a.act[l] = r.acts[l];
        int &s_in = l % 2 ? sb : sa, &s_out = l % 2 ? sa : sb;
        s_in = s_in > fq ? s_in : fq;
        s_out = s_out > fq ? s_out : fq;           // the aggregate is written to the lane's row of the output buffer
        s_out = s_out > a.jp[l] ? s_out : a.jp[l];
    }
    a.sa = sa + 4; a.sb = sb + 4;                  // + 16 bytes: rows start on different banks
    a.wfloats = round_up(off, 4);
    a.wave_floats = kRows * (a.sa + a.sb) + 3 * kRows;
    a.norm_both = r.norm == GAE_EMBED_NORM_BOTH;
    a.graph_ids = r.graph_ids; a.out = nullptr; a.ldo = 0;
    int64_t S = (r.n_out + 8191) / 8192;           // ~8 000 waves on a large set, several groups per wave on a small one
    a.S = int(S < 4 ? 4 : (S > 64 ? 64 : S));
    const int64_t waves = (r.n_out + a.S - 1) / a.S;
    return (waves + kWaves - 1) / kWaves;
}

// a launch of `kernel` with `lds` bytes of dynamic LDS; the attribute is raised once per (kernel, device)
#define GAE_GRAPHS_LAUNCH(kernel, ...)                                                                                 \
    do {                                                                                                               \
        static int configured[16] = {0};   /* per (instantiation, device): raised when a launch needs more LDS */      \
        int dev_ = 0;                                                                                                  \
        GAE_HIP(hipGetDevice(&dev_));                                                                                  \
        if (lds > 48 * 1024 && (dev_ < 0 || dev_ >= 16 || configured[dev_] < int(lds))) {                              \
            GAE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&kernel),                                       \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));                        \
            if (dev_ >= 0 && dev_ < 16) configured[dev_] = int(lds);                                                   \
        }                                                                                                              \
        hipLaunchKernelGGL(kernel, dim3(unsigned(blocks)), dim3(kWaves * 64), lds, st, __VA_ARGS__);                   \
    } while (0)

} // namespace

extern "C" int gae_embed_graphs_usable(int64_t f_in, int64_t n_layers, const int64_t *widths, int64_t max_graph_nodes)
{
    if (!widths || max_graph_nodes < 0) return 0;
    return shape_taken(f_in, n_layers, widths, max_graph_nodes, 1, nullptr, 0) ? 1 : 0;
}

extern "C" int gae_embed_graphs(const int64_t *graph_ptr, int64_t n_graphs, int64_t n_nodes, int64_t n_edges,
                                int64_t max_graph_nodes, const int32_t *indptr, const int32_t *indices,
                                const void *feat, int feat_dtype, int64_t ldf, int64_t f_in, int64_t n_layers,
                                const int64_t *widths, const float *const *weights, const int64_t *ldw,
                                const float *const *biases, const int *acts, int norm, const int64_t *graph_ids,
                                int64_t n_out, float *out, int64_t ldo, void *stream)
{
    static const char fn[] = "gae_embed_graphs";
    const Request r = {graph_ptr, n_graphs, n_nodes, n_edges, max_graph_nodes, indptr, indices, feat, feat_dtype, ldf,
                       f_in, n_layers, widths, weights, ldw, biases, acts, norm, graph_ids, n_out};
    if (const int rc = check_layers(fn, r, 1)) return rc;
    const int64_t d = widths[n_layers - 1];
    GAE_REQUIRE(ldo >= 3 * d, GAE_E_SIZE, "gae_embed_graphs: leading dimension too small (ldo %lld < 3 d = %lld)",
                (long long)ldo, (long long)(3 * d));
    if (const int rc = check_feature_rows(fn, r)) return rc;
    if (n_out == 0) return GAE_OK;
    GAE_REQUIRE(graph_ptr && out, GAE_E_NULL, "gae_embed_graphs: graph_ptr / out is NULL");
    if (const int rc = check_arrays(fn, r)) return rc;

    EmbedArgs a;
    const int64_t blocks = fill_args(r, a);
    a.out = out; a.ldo = ldo;
    GAE_REQUIRE(blocks < (int64_t(1) << 31), GAE_E_SIZE, "gae_embed_graphs: n_out = %lld is too large", (long long)n_out);
    const size_t lds = size_t(a.wfloats + kWaves * a.wave_floats) * 4;
    hipStream_t st = gae::as_stream(stream);
    if (feat_dtype == GAE_U8) GAE_GRAPHS_LAUNCH(embed_graphs_kernel<true>, a);
    else GAE_GRAPHS_LAUNCH(embed_graphs_kernel<false>, a);
    GAE_CHECK_LAUNCH("embed_graphs_kernel");
    return GAE_OK;
}

extern "C" int gae_score_graphs_usable(int64_t f_in, int64_t n_layers, const int64_t *widths, int64_t max_graph_nodes)
{
    if ((!widths && n_layers != 0) || max_graph_nodes < 0) return 0;
    return shape_taken(f_in, n_layers, widths, max_graph_nodes, 0, nullptr, 0) ? 1 : 0;
}

extern "C" int gae_score_graphs(const int64_t *graph_ptr, int64_t n_graphs, int64_t n_nodes, int64_t n_edges,
                                int64_t max_graph_nodes, const int32_t *indptr, const int32_t *indices,
                                const void *feat, int feat_dtype, int64_t ldf, int64_t f_in, int64_t n_layers,
                                const int64_t *widths, const float *const *weights, const int64_t *ldw,
                                const float *const *biases, const int *acts, int norm, const int64_t *graph_ids,
                                int64_t n_out, int exclude_self, int64_t *counts_out, double *ap_out, float *loss_out,
                                void *stream)
{
    static const char fn[] = "gae_score_graphs";
    const Request r = {graph_ptr, n_graphs, n_nodes, n_edges, max_graph_nodes, indptr, indices, feat, feat_dtype, ldf,
                       f_in, n_layers, widths, weights, ldw, biases, acts, norm, graph_ids, n_out};
    if (const int rc = check_layers(fn, r, 0)) return rc;
    GAE_REQUIRE(n_layers > 0 || feat_dtype == GAE_F32, GAE_E_DTYPE,
                "gae_score_graphs: n_layers = 0 takes the feature rows as the fp32 embedding, not dtype %d", feat_dtype);
    GAE_REQUIRE(exclude_self == 0 || exclude_self == 1, GAE_E_RANGE, "gae_score_graphs: exclude_self = %d (0 or 1)",
                exclude_self);
    if (const int rc = check_feature_rows(fn, r)) return rc;
    if (n_out == 0) return GAE_OK;
    GAE_REQUIRE(graph_ptr && counts_out && ap_out && loss_out, GAE_E_NULL,
                "gae_score_graphs: graph_ptr / counts_out / ap_out / loss_out is NULL");
    if (const int rc = check_arrays(fn, r)) return rc;

    EmbedArgs a;
    const int64_t blocks = fill_args(r, a);
    GAE_REQUIRE(blocks < (int64_t(1) << 31), GAE_E_SIZE, "gae_score_graphs: n_out = %lld is too large", (long long)n_out);
    ScoreArgs t;
    t.counts = counts_out; t.ap = ap_out; t.loss = loss_out;
    t.exclude_self = exclude_self;
    t.max_nodes = int(max_graph_nodes);
    t.rs = t.max_nodes | 1;
    t.z_in_b = a.L % 2;
    // the buffer that held Z takes the per-lane tables afterwards; the other buffer becomes the logit block
    int &s_z = t.z_in_b ? a.sb : a.sa;
    const int s_other = t.z_in_b ? a.sa : a.sb;
    if (kRows * s_z < kTabFloats) s_z = round_up((kTabFloats + kRows - 1) / kRows, 4);
    const int block = kRows * t.rs > kRows * s_other ? kRows * t.rs : kRows * s_other;
    t.block_floats = round_up(block, 4);
    a.wave_floats = kRows * s_z + t.block_floats + 3 * kRows;
    const size_t lds = size_t(a.wfloats + kWaves * a.wave_floats) * 4;
    hipStream_t st = gae::as_stream(stream);
    if (feat_dtype == GAE_U8) GAE_GRAPHS_LAUNCH(score_graphs_kernel<true>, a, t);
    else GAE_GRAPHS_LAUNCH(score_graphs_kernel<false>, a, t);
    GAE_CHECK_LAUNCH("score_graphs_kernel");
    return GAE_OK;
}
