// K19: the molecule feature of a whole resident set in ONE launch (GAE.embed_graphs, ops.embed_graphs).
//
// For every selected member graph: the complete GCN encoder (gae.py:26-31,36-45: aggregate over in-edges, Linear + bias,
// ReLU on all but the last layer) on that graph's own rows, then the README readout [mean | sum | max] over its nodes.
// The node embeddings never go to HBM: inputs are read from the dataset as it is stored (uint8 or fp32 feature rows,
// the block-diagonal CSR with global column ids), 12 d bytes are written per graph.
//
// The walk -- a wave owns S <= 64 output slots, packs consecutive graphs into groups of <= 64 rows, one atom per lane,
// the encoder of a group in two LDS buffers, the next group's loads in flight -- its aggregate / transform and its
// safety rules are graphs_walk.h's, shared with K21 (embed_bwd.hip).  K19's own tail:
//   readout     lane (slot, c) adds feature c of its graphs' rows first to last: an order that depends on the node count
//               alone
// Every output element is its own chain over the graph's own rows, so a graph's feature row has the same bits at any
// position, in any group, in any launch.  No atomics.  A slot the walk refuses gives a row of NaN.
//
// Measured (tools/embed_bench.py, profiles/r10_embed_graphs.json; 39 -> 32 -> 16, uint8 features): the 249 455 molecules of
// the ZINC-sized set in 2.43 ms of kernel time (3.1 ms per call) against 15.5 ms for batch -> encode -> readout in chunks
// of 4096 and 389 ms in chunks of 128; 9 Tflop/s, 6 % of the fp32 peak -- LDS sets 1.5 waves per SIMD and feeds every
// FMA (DESIGN.md K19 lists the levers).  175 VGPRs, no scratch (uint8 form).
//
// K20: how well every selected member graph is reconstructed (GAE.score_graphs, ops.score_graphs).  The same walk and
// the same encoder -- graphs_body below is the body of both kernels -- with a second tail in place of the readout: the
// decoder on each graph's own ordered pairs, ranked and scored in LDS.
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
#include "graphs_walk.h"

using namespace gae::walk;
using gae::v4f;

namespace {

constexpr int kWaves = 2;         // waves per block

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
    for (int l = 0; l < a.L; ++l)
        stage_layer(a.W[l], a.ldw[l], a.bias[l], a.width[l], a.width[l + 1], a.jp[l], lds + a.w_off[l],
                    lds + a.b_off[l], tid, kWaves * 64);
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
    // (K20: the logit block is sized for max_graph_nodes <= 64)
    int sn = 0, sr0 = 0;
    load_slot(a, k0, lane, avail, SCORE ? t.max_nodes : kRows, sn, sr0);

    // ---- the group that starts at slot `pos` and the loads issued for it
    constexpr int NX = U8 ? 4 : 16;                // 16-byte vectors of a feature row held in registers
    const int nvec = U8 ? (f0 + 15) / 16 : (f0 + 3) / 4;
    int pos = 0, cnt = 0, gbase = 0;
    Lane ln;
    v4f x[NX];

    auto issue = [&](int at) {
        pos = at;
        pack_group(at, lane, avail, sn, sr0, cnt, gbase, ln);
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
            lane_turn(a.indices, a.E, me);
            scale[lane] = me.sc;
            if (me.active) {
                v4f *dst = reinterpret_cast<v4f *>(bufA + lane * a.sa);
                if constexpr (U8) {
                    unpack_u8_row(x, f0, dst);
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
                switch (a.jp[l]) {                    // y replaces M; the pass mask is K21's (its switch: embed_bwd.hip)
                case 8: transform_keep<8>(Wt, bl, fi, relu, mine, mine); break;
                case 16: transform_keep<16>(Wt, bl, fi, relu, mine, mine); break;
                case 24: transform_keep<24>(Wt, bl, fi, relu, mine, mine); break;
                case 32: transform_keep<32>(Wt, bl, fi, relu, mine, mine); break;
                case 40: transform_keep<40>(Wt, bl, fi, relu, mine, mine); break;
                case 48: transform_keep<48>(Wt, bl, fi, relu, mine, mine); break;
                case 56: transform_keep<56>(Wt, bl, fi, relu, mine, mine); break;
                default: transform_keep<64>(Wt, bl, fi, relu, mine, mine); break;
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
    const char *what = "embed_graphs_kernel";
    if (feat_dtype == GAE_U8) return gae::launch_lds<&embed_graphs_kernel<true>>(what, blocks, kWaves * 64, lds, st, a);
    return gae::launch_lds<&embed_graphs_kernel<false>>(what, blocks, kWaves * 64, lds, st, a);
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
    const char *what = "score_graphs_kernel";
    if (feat_dtype == GAE_U8) return gae::launch_lds<&score_graphs_kernel<true>>(what, blocks, kWaves * 64, lds, st, a, t);
    return gae::launch_lds<&score_graphs_kernel<false>>(what, blocks, kWaves * 64, lds, st, a, t);
}
