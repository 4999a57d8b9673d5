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

template <bool U8>
__global__ __launch_bounds__(kWaves * 64) void embed_graphs_kernel(const EmbedArgs a)
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
            float *o = a.out + (k0 + pos) * a.ldo;
            for (int c = lane; c < 3 * d; c += 64) o[c] = __builtin_nanf("");
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
        {
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

int round_up(int v, int q) { return (v + q - 1) / q * q; }

// the shapes the kernel takes; `what` (may be NULL) receives the offending quantity
bool shape_taken(int64_t f_in, int64_t n_layers, const int64_t *widths, int64_t max_graph_nodes, char *what, size_t cap)
{
    if (n_layers < 1 || n_layers > kMaxLayers) {
        if (what) snprintf(what, cap, "n_layers = %lld outside 1..%d", (long long)n_layers, kMaxLayers);
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

} // namespace

extern "C" int gae_embed_graphs_usable(int64_t f_in, int64_t n_layers, const int64_t *widths, int64_t max_graph_nodes)
{
    if (!widths || max_graph_nodes < 0) return 0;
    return shape_taken(f_in, n_layers, widths, max_graph_nodes, nullptr, 0) ? 1 : 0;
}

extern "C" int gae_embed_graphs(const int64_t *graph_ptr, int64_t n_graphs, int64_t n_nodes, int64_t n_edges,
                                int64_t max_graph_nodes, const int32_t *indptr, const int32_t *indices,
                                const void *feat, int feat_dtype, int64_t ldf, int64_t f_in, int64_t n_layers,
                                const int64_t *widths, const float *const *weights, const int64_t *ldw,
                                const float *const *biases, const int *acts, int norm, const int64_t *graph_ids,
                                int64_t n_out, float *out, int64_t ldo, void *stream)
{
    GAE_REQUIRE(widths && weights && ldw && acts, GAE_E_NULL,
                "gae_embed_graphs: widths / weights / ldw / acts is NULL");
    GAE_REQUIRE(n_graphs >= 0 && n_nodes >= 0 && n_edges >= 0 && n_out >= 0 && max_graph_nodes >= 0, GAE_E_SIZE,
                "gae_embed_graphs: negative n_graphs = %lld, n_nodes = %lld, n_edges = %lld, n_out = %lld or "
                "max_graph_nodes = %lld", (long long)n_graphs, (long long)n_nodes, (long long)n_edges, (long long)n_out,
                (long long)max_graph_nodes);
    GAE_REQUIRE(n_nodes < (int64_t(1) << 31) && n_edges < (int64_t(1) << 31), GAE_E_SIZE,
                "gae_embed_graphs: n_nodes = %lld or n_edges = %lld beyond the int32 CSR", (long long)n_nodes,
                (long long)n_edges);
    char what[160];
    GAE_REQUIRE(shape_taken(f_in, n_layers, widths, max_graph_nodes, what, sizeof what), GAE_E_RANGE,
                "gae_embed_graphs: %s", what);
    GAE_REQUIRE(norm == GAE_EMBED_NORM_NONE || norm == GAE_EMBED_NORM_BOTH, GAE_E_RANGE,
                "gae_embed_graphs: unknown norm code %d (0 = none, 1 = both)", norm);
    GAE_REQUIRE(feat_dtype == GAE_F32 || feat_dtype == GAE_U8, GAE_E_DTYPE,
                "gae_embed_graphs: feature dtype %d (GAE_F32 or GAE_U8)", feat_dtype);
    for (int64_t l = 0; l < n_layers; ++l) {
        GAE_REQUIRE(acts[l] == GAE_ACT_IDENTITY || acts[l] == GAE_ACT_RELU, GAE_E_DTYPE,
                    "gae_embed_graphs: unknown activation code %d of layer %lld", acts[l], (long long)l);
        GAE_REQUIRE(weights[l], GAE_E_NULL, "gae_embed_graphs: the weight of layer %lld is NULL", (long long)l);
        GAE_REQUIRE(ldw[l] >= (l ? widths[l - 1] : f_in), GAE_E_SIZE,
                    "gae_embed_graphs: leading dimension ldw = %lld of layer %lld below its input width",
                    (long long)ldw[l], (long long)l);
    }
    const int64_t d = widths[n_layers - 1];
    GAE_REQUIRE(ldo >= 3 * d, GAE_E_SIZE, "gae_embed_graphs: leading dimension too small (ldo %lld < 3 d = %lld)",
                (long long)ldo, (long long)(3 * d));
    const int64_t row_elems = feat_dtype == GAE_U8 ? (f_in + 15) / 16 * 16 : (f_in + 3) / 4 * 4;
    GAE_REQUIRE(ldf >= row_elems, GAE_E_SIZE,
                "gae_embed_graphs: feature rows of ldf = %lld elements, %lld needed (whole 16-byte vectors)",
                (long long)ldf, (long long)row_elems);
    if (n_out == 0) return GAE_OK;
    GAE_REQUIRE(graph_ptr && out, GAE_E_NULL, "gae_embed_graphs: graph_ptr / out is NULL");
    GAE_REQUIRE(n_nodes == 0 || (indptr && feat), GAE_E_NULL, "gae_embed_graphs: indptr / feat is NULL");
    GAE_REQUIRE(n_edges == 0 || indices, GAE_E_NULL, "gae_embed_graphs: indices is NULL");
    const int64_t row_bytes = ldf * (feat_dtype == GAE_U8 ? 1 : 4);
    GAE_REQUIRE(n_nodes == 0 || (gae::aligned16(feat) && row_bytes % 16 == 0), GAE_E_ALIGN,
                "gae_embed_graphs: feature rows must start on 16-byte boundaries (pointer and ldf)");

    EmbedArgs a;
    a.graph_ptr = graph_ptr; a.indptr = indptr; a.indices = indices; a.feat = feat; a.ldf = ldf;
    a.G = n_graphs; a.N = n_nodes; a.E = n_edges; a.B = n_out;
    a.L = int(n_layers);
    a.width[0] = int(f_in);
    for (int l = 0; l < a.L; ++l) a.width[l + 1] = int(widths[l]);
    int off = 0;
    for (int l = 0; l < kMaxLayers; ++l) {
        a.jp[l] = a.w_off[l] = a.b_off[l] = a.act[l] = 0;
        a.W[l] = nullptr; a.bias[l] = nullptr; a.ldw[l] = 0;
    }
    int sa = 0, sb = 0;
    for (int l = 0; l < a.L; ++l) {
        const int fq = round_up(a.width[l], 4);    // the input (and its aggregate) in whole 16-byte vectors
        a.jp[l] = round_up(a.width[l + 1], 8);
        a.w_off[l] = off; off += a.width[l] * a.jp[l];
        a.b_off[l] = off; off += a.jp[l];
        a.W[l] = weights[l]; a.ldw[l] = ldw[l]; a.bias[l] = biases ? biases[l] : nullptr; a.act[l] = acts[l];
        int &s_in = l % 2 ? sb : sa, &s_out = l % 2 ? sa : sb;
        s_in = s_in > fq ? s_in : fq;
        s_out = s_out > fq ? s_out : fq;           // the aggregate is written to the lane's row of the output buffer
        s_out = s_out > a.jp[l] ? s_out : a.jp[l];
    }
    a.sa = sa + 4; a.sb = sb + 4;                  // + 16 bytes: rows start on different banks
    a.wfloats = round_up(off, 4);
    a.wave_floats = kRows * (a.sa + a.sb) + 3 * kRows;
    a.norm_both = norm == GAE_EMBED_NORM_BOTH;
    a.graph_ids = graph_ids; a.out = out; a.ldo = ldo;
    int64_t S = (n_out + 8191) / 8192;             // ~8 000 waves on a large set, several groups per wave on a small one
    a.S = int(S < 4 ? 4 : (S > 64 ? 64 : S));
    const int64_t waves = (n_out + a.S - 1) / a.S;
    const int64_t blocks = (waves + kWaves - 1) / kWaves;
    GAE_REQUIRE(blocks < (int64_t(1) << 31), GAE_E_SIZE, "gae_embed_graphs: n_out = %lld is too large", (long long)n_out);
    const size_t lds = size_t(a.wfloats + kWaves * a.wave_floats) * 4;
    hipStream_t st = gae::as_stream(stream);
#define GAE_EMBED_LAUNCH(U8)                                                                                           \
    do {                                                                                                               \
        static int configured[16] = {0};   /* per (instantiation, device): raised when a launch needs more LDS */      \
        int dev_ = 0;                                                                                                  \
        GAE_HIP(hipGetDevice(&dev_));                                                                                  \
        if (lds > 48 * 1024 && (dev_ < 0 || dev_ >= 16 || configured[dev_] < int(lds))) {                              \
            GAE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&embed_graphs_kernel<U8>),                      \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));                        \
            if (dev_ >= 0 && dev_ < 16) configured[dev_] = int(lds);                                                   \
        }                                                                                                              \
        hipLaunchKernelGGL((embed_graphs_kernel<U8>), dim3(unsigned(blocks)), dim3(kWaves * 64), lds, st, a);          \
    } while (0)
    if (feat_dtype == GAE_U8) GAE_EMBED_LAUNCH(true);
    else GAE_EMBED_LAUNCH(false);
#undef GAE_EMBED_LAUNCH
    GAE_CHECK_LAUNCH("embed_graphs_kernel");
    return GAE_OK;
}
