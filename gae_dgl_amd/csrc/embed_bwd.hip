// K21: the backward of K19 (gae_embed_graphs_bwd; ops.embed_graphs under autograd, GAE.embed_graphs(grad=True)).
//
// d_out [B, 3 d] = the gradient of a loss with respect to the molecule features [mean | sum | max]; the kernel leaves
// the weight and bias gradients of every encoder layer behind and nothing else: per group of <= 64 rows it runs the
// encoder AGAIN in LDS (nothing per node is saved between the forward and the backward call), then walks the layers
// last to first.  The walk -- a wave owns S consecutive slots, packs consecutive graphs into groups of <= 64 rows, one
// atom per lane, the next group's row bounds (and uint8 feature rows) in flight while this one computes -- is K19's:
// both kernels call the one copy in graphs_walk.h, which describes its layout, loads and safety rules.
//
// Per group.
//   forward     K19's aggregate / transform_keep (graphs_walk.h: the same fmaf chains, k ascending); every layer's aggregated input
//               M_l [64][width_l] STAYS in LDS, the activations go through one buffer T; a hidden layer's ReLU pass mask
//               is one 64-bit word per lane (widths <= 64, a lane holds one atom's row)
//   readout     lane (slot, c) walks column c of its graphs' rows of Z: the maximum and the LOWEST row attaining it, then
//               writes dZ[r][c] = d_sum[c] + d_mean[c] / n + (r == r* ? d_max[c] : 0) for the graph's rows
//   per layer   dY = dH (.) mask in place;  db_l += sum_r dY[r] (lane j adds column j first row to last);
//               dW_l += dY^T M_l on v_mfma_f32_32x32x2_f32: the product reduces over the rows = across lanes, so unlike
//               the forward's atoms-as-lanes chains it belongs on the matrix core; A = dY, B = M_l, one float each per
//               step read from LDS, two rows per step, rows at or above the group's row count read as zero.  The 32 x 32
//               tiles of all layers (at most 8: 128 registers) and the db sums stay in registers across all groups of
//               the wave.  dM = dY W_l with lane = row (fmaf chains over j ascending, broadcast reads of W_l in its
//               stored [j][k] order, staged beside the forward's transposed copy), then dH_{l-1} = A^T dM
//   A^T         the CSR stores in-edges, so row u needs sum_r mult(r, u) sc_r sc_u dM[r]: a GATHER.  Once per group lane
//               u scans the neighbour table of its graph's rows (in LDS; rows longer than four entries continue from the
//               CSR) and keeps its first four (row, multiplicity x scale) pairs in registers and the rows beyond them as
//               a 64-bit mask; every layer adds them in ascending row order.  Directed sets, repeated edges and self
//               loops are what the multiplicity is for
// No LDS or global float atomics.  Every wave writes ONE partial per parameter into the workspace; a second stage adds
// the partials in the library's one order (gae::sum_partials, through gae::launch_partials_reduce) and writes dW / db.
// Same call, same bits.
//
// Safety: the walk's rules (graphs_walk.h).  A refused slot (bad id, bad range, more than 64 rows) and an empty graph contribute nothing; a
// row pointer outside [0, E] reads as an empty row; a column id outside the graph's own rows is skipped.
//
// LDS per wave: sum_l 64 x (width_l rounded up to 4, + 4) floats of M_l, two buffers of 64 x (widest layer + 4) floats
// and 4.25 KB of tables; per block the weights in both orientations.  A block takes as many waves (<= 4) as fit 160 KB,
// a call of at most 256 waves one wave per block (it spreads over the CUs instead):
//   39 -> 32 -> 16              9.1 KB + 46.25 KB per wave: 3 waves, 147.8 KB per block
//   39 -> 16                    2.5 KB + 37.25 KB per wave: 4 waves, 151.5 KB
//   39 -> 64 -> 32 -> 16        30.2 KB + 75.25 KB per wave: 1 wave, 105.4 KB
//   39 -> 32 -> 32 -> 32 -> 8   23.3 KB + 64.25 KB per wave: 2 waves, 151.8 KB
// so one block per CU and at most one wave per SIMD (0.25 .. 1): LDS, not registers, sets the occupancy, and the
// compiler is given the whole file for it -- 256 VGPRs + 233 AGPRs (uint8 form), 256 + 199 (fp32 form; its feature rows
// are loaded at the group's turn, four vectors at a time), no scratch in either (kernel-resource-usage report of hipcc).
// gae_embed_graphs_bwd_usable refuses what does not fit one wave or needs more than 8 tiles: four layers of width 64
// (16 tiles, 219 KB) and 39 -> 64 -> 64 -> 64 (12 tiles) are outside, 39 -> 64 -> 64 (8 tiles, 108.5 KB) is inside.
// Time: DESIGN.md K21 (tools/embed_bwd_bench.py).
#include "graphs_walk.h"

using namespace gae::walk;
using gae::v4f;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMaxWaves = 4;      // waves per block
constexpr int kMaxTiles = 8;      // 32 x 32 accumulator tiles of all layers
constexpr int kLdsCap = 160 * 1024;

struct BwdArgs {
    const int64_t *graph_ptr;
    const int32_t *indptr, *indices;
    const void *feat;
    int64_t ldf;
    int64_t G, N, E, B;
    int L;
    int width[kMaxLayers + 1];    // f_in, then every layer's output width
    int jp[kMaxLayers];           // outputs computed by layer l: its width rounded up to 8
    int kp[kMaxLayers];           // columns of dM of layer l: its input width rounded up to 8
    int wt_off[kMaxLayers], wk_off[kMaxLayers], b_off[kMaxLayers];   // staged W^T [f_in][jp], W [f_out][kp], bias [jp]
    const float *W[kMaxLayers];
    int64_t ldw[kMaxLayers];
    const float *bias[kMaxLayers];
    int act[kMaxLayers];
    int norm_both;
    const int64_t *graph_ids;
    const float *d_out;
    int64_t ldd;
    float *part;                  // [n_partials][P]
    int64_t P;                    // floats of one partial
    int pw_off[kMaxLayers], pb_off[kMaxLayers];
    int want[kMaxLayers];         // dW or db of the layer is asked for
    int l_stop;                   // the lowest layer that is
    int S;                        // output slots per wave
    int sm[kMaxLayers], m_off[kMaxLayers];   // row stride / float offset of M_l in a wave's LDS
    int st, t_off, d_off, tab_off;           // the two [64][st] buffers, the tables
    int wfloats, wave_floats;
    int ntiles, tl[kMaxTiles], tj[kMaxTiles], tk[kMaxTiles];         // tile t: layer, 32-row block of j, of k
};

// float offsets of a wave's tables
enum { kTabScale = 0, kTabBase = 64, kTabCount = 128, kTabNb = 192, kTabE0 = 448, kTabE1 = 512, kTabMask = 576,
       kTabFloats = 576 + 2 * kRows * kMaxLayers };

// dM = dY W of the lane's row: dY (fo values) is read from `mine`, dM (KP values, zero beyond the input width) replaces it
template <int KP>
__device__ __forceinline__ void backprop(const float *Wk, int fo, float *mine)
{
    float m[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) m[k] = 0.f;
#pragma unroll 1
    for (int j = 0; j < fo; ++j) {
        const float dy = mine[j];
        const v4f *w = reinterpret_cast<const v4f *>(Wk + j * KP);
#pragma unroll
        for (int q = 0; q < KP / 4; ++q) {
            const v4f wv = w[q];
#pragma unroll
            for (int i = 0; i < 4; ++i) m[4 * q + i] = fmaf(dy, wv[i], m[4 * q + i]);
        }
    }
#pragma unroll
    for (int q = 0; q < KP / 4; ++q) {
        const v4f v = {m[4 * q], m[4 * q + 1], m[4 * q + 2], m[4 * q + 3]};
        *reinterpret_cast<v4f *>(mine + 4 * q) = v;
    }
}

// how often group row r lists group row u (global column id gcol): its four table entries, then its CSR tail
__device__ __forceinline__ int mult_of(const BwdArgs &a, const int *tab, int r, int u, int gcol)
{
    const int *nb = tab + kTabNb + 4 * r;
    int m = (nb[0] == u) + (nb[1] == u) + (nb[2] == u) + (nb[3] == u);
    const int e0 = tab[kTabE0 + r], e1 = tab[kTabE1 + r];
    if (e1 - e0 > kRegNb)
        for (int e = e0 + kRegNb; e < e1; ++e) m += a.indices[e] == gcol;
    return m;
}

// one 32 x 32 tile of dW += dY^T M over the group's rows, two rows per v_mfma_f32_32x32x2_f32: lane (h, c) feeds
// A[j0 + c][row 2 s + h] and B[row 2 s + h][k0 + c]; what lies outside the group's rows or the layer's widths is zero
__device__ __forceinline__ f32x16 wgrad_tile(const float *Y, int sy, const float *M, int sm, int rows, int j0, int k0,
                                             int fo, int fi, int lane, f32x16 acc)
{
    const int h = lane >> 5, c = lane & 31;
    const bool ja = j0 + c < fo, ka = k0 + c < fi;
    const float *yp = Y + (ja ? j0 + c : 0), *mp = M + (ka ? k0 + c : 0);

    for (int s = 0; 2 * s < rows; ++s) {
        const int r = 2 * s + h;                     // <= 63: inside both buffers
        const bool ra = r < rows;
        const float yv = yp[r * sy], mv = mp[r * sm];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ra && ja ? yv : 0.f, ra && ka ? mv : 0.f, acc, 0, 0, 0);
    }
    return acc;
}

template <bool U8>
__global__ __launch_bounds__(kMaxWaves * 64) void embed_graphs_bwd_kernel(const BwdArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, nthreads = blockDim.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform: what hangs on it stays scalar

    // ---- the weights of all layers, once per block: W^T zero padded to [f_in][jp] and W zero padded to [f_out][kp]
    for (int l = 0; l < a.L; ++l) {
        const int jp = a.jp[l], kp = a.kp[l], fi = a.width[l], fo = a.width[l + 1];
        const float *W = a.W[l];
        const int64_t ldw = a.ldw[l];
        stage_layer(W, ldw, a.bias[l], fi, fo, jp, lds + a.wt_off[l], lds + a.b_off[l], tid, nthreads);
        if (l > a.l_stop) {
            float *dk = lds + a.wk_off[l];
            for (int idx = tid; idx < fo * kp; idx += nthreads) {
                const int j = idx / kp, k = idx - j * kp;
                const float v = W[k < fi ? j * ldw + k : 0];
                dk[idx] = k < fi ? v : 0.f;
            }
        }
    }
    __syncthreads();

    float *wbase = lds + a.wfloats + wave * a.wave_floats;
    float *T = wbase + a.t_off, *D = wbase + a.d_off;
    float *scale = wbase + a.tab_off + kTabScale;
    int *tab = reinterpret_cast<int *>(wbase + a.tab_off);
    int *mbase = tab + kTabBase, *mcount = tab + kTabCount;
    uint64_t *masks = reinterpret_cast<uint64_t *>(tab + kTabMask);
    const int st = a.st;

    const int64_t wave_id = int64_t(blockIdx.x) * (nthreads >> 6) + wave;
    const int64_t k0 = wave_id * a.S;
    const int avail = k0 >= a.B ? 0 : int(a.B - k0 < a.S ? a.B - k0 : a.S);
    const int d = a.width[a.L];
    const int f0 = a.width[0];

    f32x16 acc[kMaxTiles];
#pragma unroll
    for (int t = 0; t < kMaxTiles; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
    float dbacc[kMaxLayers] = {0.f, 0.f, 0.f, 0.f};

    // ---- this wave's slots: lane t holds slot t (graph id -> node range), loaded once
    int sn = 0, sr0 = 0;
    load_slot(a, k0, lane, avail, kRows, sn, sr0);

    // ---- the group that starts at slot `pos` and the loads issued for it
    constexpr int NX = 4;                          // 16-byte vectors of a uint8 feature row held in registers
    const int nvec = U8 ? (f0 + 15) / 16 : (f0 + 3) / 4;
    int pos = 0, cnt = 0, gbase = 0, grows = 0;
    Lane ln;
    v4f x[NX];

    auto issue = [&](int at) {
        pos = at;
        grows = pack_group(at, lane, avail, sn, sr0, cnt, gbase, ln);
        if (ln.active) {
            const int64_t gr = int64_t(ln.g0) + (lane - ln.mb);
            ln.e0 = a.indptr[gr];
            ln.e1 = a.indptr[gr + 1];
            if constexpr (U8) {                      // (an fp32 row is 16 vectors: loaded at the group's turn instead)
                const v4f *row = reinterpret_cast<const v4f *>(static_cast<const char *>(a.feat) + gr * a.ldf);
#pragma unroll
                for (int q = 0; q < NX; ++q)
                    if (q < nvec) x[q] = row[q];
            }
        }
    };

    issue(0);
    while (pos < avail) {
        if (cnt == 0) {                              // a slot that cannot be taken contributes nothing
            issue(pos + 1);
            continue;
        }
        // ---- the group's turn: its registers go to LDS
        const Lane cur = ln;
        const int cpos = pos, ccnt = cnt, crows = grows;
        Lane me = cur;
        {
            const int mi = lane - cpos;
            if (mi >= 0 && mi < ccnt) { mbase[mi] = gbase; mcount[mi] = sn; }
            lane_turn(a.indices, a.E, me);
#pragma unroll
            for (int q = 0; q < kRegNb; ++q) tab[kTabNb + 4 * lane + q] = me.nb[q];
            tab[kTabE0 + lane] = me.e0;
            tab[kTabE1 + lane] = me.e1;
            scale[lane] = me.sc;
            if (me.active) {
                v4f *dst = reinterpret_cast<v4f *>(T + lane * st);
                if constexpr (U8) {
                    unpack_u8_row(x, f0, dst);
                } else {                             // an fp32 row is 16 vectors: loaded here, four at a time
                    const int64_t gr = int64_t(me.g0) + (lane - me.mb);
                    const v4f *row = reinterpret_cast<const v4f *>(static_cast<const char *>(a.feat) + gr * a.ldf * 4);
#pragma unroll 1
                    for (int c0 = 0; c0 < nvec; c0 += 4) {
                        v4f v[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) v[q] = row[c0 + q < nvec ? c0 + q : c0];
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (c0 + q < nvec) {
#pragma unroll
                                for (int i = 0; i < 4; ++i) v[q][i] = 4 * (c0 + q) + i < f0 ? v[q][i] : 0.f;   // pad columns are not data
                                dst[c0 + q] = v[q];
                            }
                    }
                }
            }
            wave_sync();
        }
        issue(cpos + ccnt);                          // the next group's loads are in flight while the layers run

        // ---- the rows that list this lane's row, ascending: four (row, multiplicity x scale) pairs, the rest as a mask
        int on[kRegNb] = {-1, -1, -1, -1};
        float oc[kRegNb] = {0.f, 0.f, 0.f, 0.f};
        uint64_t rest = 0;
        const int gcol = me.g0 + (lane - me.mb);
        if (me.active && a.l_stop < a.L - 1) {
            int found = 0;
            for (int r = me.mb; r < me.mb + me.mn; ++r) {
                const int mu = mult_of(a, tab, r, lane, gcol);
                if (mu == 0) continue;
                const float coef = float(mu) * (a.norm_both ? scale[r] : 1.f);
                if (found >= kRegNb) rest |= 1ull << (r - me.mb);
#pragma unroll
                for (int q = 0; q < kRegNb; ++q)
                    if (q == found) { on[q] = r; oc[q] = coef; }
                ++found;
            }
        }

        // ---- forward, M_l kept
        for (int l = 0; l < a.L; ++l) {
            const int fi = a.width[l];
            float *Ml = wbase + a.m_off[l];
            const int sm = a.sm[l];
            if (me.active) aggregate(a, me, lane, fi, T, st, Ml, sm, scale);
            wave_sync();                             // every lane has read its neighbours' rows of T
            uint64_t mask = ~0ull;
            if (me.active) {
                const float *Wt = lds + a.wt_off[l], *bl = lds + a.b_off[l];
                const bool relu = a.act[l] == GAE_ACT_RELU;
                const float *mrow = Ml + lane * sm;
                float *yrow = T + lane * st;
                // (the switch is written out here and in embed.hip: behind one shared dispatcher the compiler rescheduled
                // 760 of this kernel's 10 500 instructions, with nothing to gain)
                switch (a.jp[l]) {
                case 8: mask = transform_keep<8>(Wt, bl, fi, relu, mrow, yrow); break;
                case 16: mask = transform_keep<16>(Wt, bl, fi, relu, mrow, yrow); break;
                case 24: mask = transform_keep<24>(Wt, bl, fi, relu, mrow, yrow); break;
                case 32: mask = transform_keep<32>(Wt, bl, fi, relu, mrow, yrow); break;
                case 40: mask = transform_keep<40>(Wt, bl, fi, relu, mrow, yrow); break;
                case 48: mask = transform_keep<48>(Wt, bl, fi, relu, mrow, yrow); break;
                case 56: mask = transform_keep<56>(Wt, bl, fi, relu, mrow, yrow); break;
                default: mask = transform_keep<64>(Wt, bl, fi, relu, mrow, yrow); break;
                }
            }
            masks[l * kRows + lane] = mask;
            wave_sync();
        }

        // ---- readout backward: Z = T; lane (slot, c) owns column c of its graphs
        {
            int DP = 1;
            while (DP < d) DP <<= 1;
            const int c = lane & (DP - 1), slot = lane / DP, RS = 64 / DP;
            if (c < d) {
                for (int m = slot; m < ccnt; m += RS) {
                    const int b = mbase[m], n = mcount[m];
                    if (n == 0) continue;
                    const float *go = a.d_out + (k0 + cpos + m) * a.ldd;
                    const float gmean = go[c], gsum = go[d + c], gmax = go[2 * d + c];
                    float mx = T[b * st + c];
                    int rs = b;
                    for (int r = b + 1; r < b + n; ++r) {
                        const float v = T[r * st + c];
                        if (v > mx) { mx = v; rs = r; }          // strict: the lowest row attaining the maximum
                    }
                    const float base = gsum + gmean / float(n);
                    for (int r = b; r < b + n; ++r) D[r * st + c] = r == rs ? base + gmax : base;
                }
            }
            wave_sync();
        }

        // ---- the layers, last to first: dH of the layer is in P
        float *P = D, *Q = T;
        for (int l = a.L - 1; l >= a.l_stop; --l) {
            const int fi = a.width[l], fo = a.width[l + 1];
            const float *Ml = wbase + a.m_off[l];
            const int sm = a.sm[l];
            if (me.active) {                         // dY = dH (.) mask in place, zeros up to jp
                const uint64_t mask = masks[l * kRows + lane];
                v4f *row = reinterpret_cast<v4f *>(P + lane * st);
                for (int q = 0; q < a.jp[l] / 4; ++q) {
                    v4f v = row[q];
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = (4 * q + i < fo && ((mask >> (4 * q + i)) & 1)) ? v[i] : 0.f;
                    row[q] = v;
                }
            }
            wave_sync();
            if (a.want[l]) {
                if (lane < fo) {
                    float s = 0.f;
                    for (int r = 0; r < crows; ++r) s += P[r * st + lane];
#pragma unroll
                    for (int q = 0; q < kMaxLayers; ++q)
                        if (q == l) dbacc[q] += s;
                }
#pragma unroll
                for (int t = 0; t < kMaxTiles; ++t)
                    if (t < a.ntiles && a.tl[t] == l)
                        acc[t] = wgrad_tile(P, st, Ml, sm, crows, 32 * a.tj[t], 32 * a.tk[t], fo, fi, lane, acc[t]);
            }
            if (l > a.l_stop) {
                wave_sync();                         // the tiles have read every row of dY
                if (me.active) {
                    const float *Wk = lds + a.wk_off[l];
                    float *mine = P + lane * st;
                    switch (a.kp[l]) {
                    case 8: backprop<8>(Wk, fo, mine); break;
                    case 16: backprop<16>(Wk, fo, mine); break;
                    case 24: backprop<24>(Wk, fo, mine); break;
                    case 32: backprop<32>(Wk, fo, mine); break;
                    case 40: backprop<40>(Wk, fo, mine); break;
                    case 48: backprop<48>(Wk, fo, mine); break;
                    case 56: backprop<56>(Wk, fo, mine); break;
                    default: backprop<64>(Wk, fo, mine); break;
                    }
                }
                wave_sync();
                if (me.active) {                     // dH_{l-1} = A^T dM: the rows that list this one, ascending
                    for (int c = 0; c < (fi + 3) / 4; ++c) {
                        v4f s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int q = 0; q < kRegNb; ++q)
                            if (on[q] >= 0) {
                                const v4f v = *reinterpret_cast<const v4f *>(P + on[q] * st + 4 * c);
#pragma unroll
                                for (int i = 0; i < 4; ++i) s[i] = fmaf(oc[q], v[i], s[i]);
                            }
                        uint64_t m = rest;
                        while (m) {
                            const int r = me.mb + __builtin_ctzll(m);
                            m &= m - 1;
                            const float coef = float(mult_of(a, tab, r, lane, gcol)) * (a.norm_both ? scale[r] : 1.f);
                            const v4f v = *reinterpret_cast<const v4f *>(P + r * st + 4 * c);
#pragma unroll
                            for (int i = 0; i < 4; ++i) s[i] = fmaf(coef, v[i], s[i]);
                        }
                        if (a.norm_both) s *= me.sc;
                        *reinterpret_cast<v4f *>(Q + lane * st + 4 * c) = s;
                    }
                }
                wave_sync();
                float *t = P; P = Q; Q = t;
            }
        }
        wave_sync();                                 // the next group's turn overwrites the tables and T
    }

    // ---- this wave's partial: one value per parameter (zeros from a wave without slots)
    float *part = a.part + wave_id * a.P;
#pragma unroll
    for (int t = 0; t < kMaxTiles; ++t)
        if (t < a.ntiles && a.want[a.tl[t]]) {
            const int l = a.tl[t], fi = a.width[l], fo = a.width[l + 1];
            const int k = 32 * a.tk[t] + (lane & 31);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int j = 32 * a.tj[t] + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
                if (j < fo && k < fi) part[a.pw_off[l] + j * fi + k] = acc[t][i];
            }
        }
#pragma unroll
    for (int l = 0; l < kMaxLayers; ++l)
        if (l < a.L && a.want[l] && lane < a.width[l + 1]) part[a.pb_off[l] + lane] = dbacc[l];
}

// the LDS layout, the tiles and the partial's layout of an encoder f_in -> widths (shape_taken holds); returns the
// waves per block that fit (0: the encoder is refused) and in `what` the reason
int plan_shapes(int64_t f_in, int64_t n_layers, const int64_t *widths, BwdArgs &a, char *what, size_t cap)
{
    a.L = int(n_layers);
    a.width[0] = int(f_in);
    for (int l = 0; l < a.L; ++l) a.width[l + 1] = int(widths[l]);
    for (int l = a.L + 1; l <= kMaxLayers; ++l) a.width[l] = 0;
    for (int l = 0; l < kMaxLayers; ++l) {
        a.jp[l] = a.kp[l] = a.wt_off[l] = a.wk_off[l] = a.b_off[l] = a.act[l] = a.want[l] = 0;
        a.pw_off[l] = a.pb_off[l] = a.sm[l] = a.m_off[l] = 0;
        a.W[l] = nullptr; a.bias[l] = nullptr; a.ldw[l] = 0;
    }
    for (int t = 0; t < kMaxTiles; ++t) a.tl[t] = a.tj[t] = a.tk[t] = -1;
    int off = 0, moff = 0, st = round_up(a.width[0], 4), nt = 0, P = 0;
    for (int l = 0; l < a.L; ++l) {
        const int fi = a.width[l], fo = a.width[l + 1];
        a.jp[l] = round_up(fo, 8);
        a.kp[l] = round_up(fi, 8);
        a.wt_off[l] = off; off += fi * a.jp[l];
        a.wk_off[l] = off; off += l ? fo * a.kp[l] : 0;          // (dM of layer 0 is never formed)
        a.b_off[l] = off; off += a.jp[l];
        a.sm[l] = round_up(fi, 4) + 4;                           // + 16 bytes: rows start on different banks
        a.m_off[l] = moff; moff += kRows * a.sm[l];
        st = st > a.jp[l] ? st : a.jp[l];          // T / D hold X, every Y_l and dH_l (jp) and every dM_l, l > 0 (kp)
        if (l && st < a.kp[l]) st = a.kp[l];
        for (int jb = 0; jb < (fo + 31) / 32; ++jb)
            for (int kb = 0; kb < (fi + 31) / 32; ++kb) {
                if (nt < kMaxTiles) { a.tl[nt] = l; a.tj[nt] = jb; a.tk[nt] = kb; }
                ++nt;
            }
        a.pw_off[l] = P; P += fo * fi;
        a.pb_off[l] = P; P += fo;
    }
    a.ntiles = nt < kMaxTiles ? nt : kMaxTiles;
    a.P = P;
    a.st = st + 4;
    a.t_off = moff;
    a.d_off = moff + kRows * a.st;
    a.tab_off = moff + 2 * kRows * a.st;
    a.wfloats = round_up(off, 4);
    a.wave_floats = a.tab_off + kTabFloats;
    if (nt > kMaxTiles) {
        if (what)
            snprintf(what, cap, "the weight gradients of %lld layers need %d accumulator tiles of 32 x 32, at most %d "
                     "stay in registers", (long long)n_layers, nt, kMaxTiles);
        return 0;
    }
    const int64_t room = kLdsCap / 4 - a.wfloats;
    const int nw = room < a.wave_floats ? 0 : int(room / a.wave_floats);
    if (nw == 0 && what)
        snprintf(what, cap, "LDS of %lld bytes per block (every layer's aggregated input and the weights twice), at "
                 "most %d", (long long)(a.wfloats + a.wave_floats) * 4, kLdsCap);
    return nw > kMaxWaves ? kMaxWaves : nw;
}

// slots per wave, waves per block and blocks of a call over n_out slots
struct Grid { int S, nw; int64_t blocks, n_partials; };

Grid plan_grid(int64_t n_out, int nw_max)
{
    Grid g;
    const int64_t S = (n_out + 2047) / 2048;       // ~2 000 waves on a large set: the partials stay a few tens of MB
    g.S = int(S < 4 ? 4 : (S > 64 ? 64 : S));
    const int64_t waves = (n_out + g.S - 1) / g.S;
    g.nw = waves <= 256 ? 1 : nw_max;              // a small call spreads over the CUs, a large one shares the weights
    g.blocks = (waves + g.nw - 1) / g.nw;
    g.n_partials = g.blocks * g.nw;
    return g;
}

// an upper bound of plan_grid's n_partials that grows with n_out
int64_t partials_bound(int64_t n_out)
{
    const int64_t small = (n_out + 3) / 4 < 2048 ? (n_out + 3) / 4 : 2048, large = (n_out + 63) / 64;
    return (small > large ? small : large) + kMaxWaves;
}

} // namespace

extern "C" int gae_embed_graphs_bwd_usable(int64_t f_in, int64_t n_layers, const int64_t *widths, int64_t max_graph_nodes)
{
    if (!widths || max_graph_nodes < 0) return 0;
    if (!shape_taken(f_in, n_layers, widths, max_graph_nodes, 1, nullptr, 0)) return 0;
    BwdArgs a;
    return plan_shapes(f_in, n_layers, widths, a, nullptr, 0) > 0 ? 1 : 0;
}

extern "C" int64_t gae_embed_graphs_bwd_workspace_bytes(int64_t f_in, int64_t n_layers, const int64_t *widths,
                                                        int64_t n_out)
{
    GAE_REQUIRE(widths, GAE_E_NULL, "gae_embed_graphs_bwd_workspace_bytes: widths is NULL");
    GAE_REQUIRE(n_out >= 0, GAE_E_SIZE, "gae_embed_graphs_bwd_workspace_bytes: negative n_out = %lld", (long long)n_out);
    char what[200];
    GAE_REQUIRE(shape_taken(f_in, n_layers, widths, 0, 1, what, sizeof what), GAE_E_RANGE,
                "gae_embed_graphs_bwd_workspace_bytes: %s", what);
    BwdArgs a;
    GAE_REQUIRE(plan_shapes(f_in, n_layers, widths, a, what, sizeof what) > 0, GAE_E_RANGE,
                "gae_embed_graphs_bwd_workspace_bytes: %s", what);
    return partials_bound(n_out) * a.P * 4;
}

extern "C" int gae_embed_graphs_bwd(const int64_t *graph_ptr, int64_t n_graphs, int64_t n_nodes, int64_t n_edges,
                                    int64_t max_graph_nodes, const int32_t *indptr, const int32_t *indices,
                                    const void *feat, int feat_dtype, int64_t ldf, int64_t f_in, int64_t n_layers,
                                    const int64_t *widths, const float *const *weights, const int64_t *ldw,
                                    const float *const *biases, const int *acts, int norm, const int64_t *graph_ids,
                                    int64_t n_out, const float *d_out, int64_t ldd, float *const *dW,
                                    const int64_t *lddw, float *const *db, void *workspace, int64_t workspace_bytes,
                                    void *stream)
{
    static const char fn[] = "gae_embed_graphs_bwd";
    const Request r = {graph_ptr, n_graphs, n_nodes, n_edges, max_graph_nodes, indptr, indices, feat, feat_dtype, ldf,
                       f_in, n_layers, widths, weights, ldw, biases, acts, norm, graph_ids, n_out};
    if (const int rc = check_layers(fn, r, 1)) return rc;
    GAE_REQUIRE(dW && lddw && db, GAE_E_NULL, "%s: the table dW / lddw / db is NULL (an ENTRY may be NULL: not wanted)",
                fn);
    char what[200];
    BwdArgs a;
    const int nw_max = plan_shapes(f_in, n_layers, widths, a, what, sizeof what);
    GAE_REQUIRE(nw_max > 0, GAE_E_RANGE, "%s: %s", fn, what);
    bool any = false;
    for (int64_t l = 0; l < n_layers; ++l) {
        GAE_REQUIRE(!dW[l] || lddw[l] >= (l ? widths[l - 1] : f_in), GAE_E_SIZE,
                    "%s: leading dimension lddw = %lld of layer %lld below its input width", fn, (long long)lddw[l],
                    (long long)l);
        any = any || dW[l] || db[l];
    }
    const int64_t d = widths[n_layers - 1];
    GAE_REQUIRE(ldd >= 3 * d, GAE_E_SIZE, "%s: leading dimension too small (ldd %lld < 3 d = %lld)", fn, (long long)ldd,
                (long long)(3 * d));
    if (const int rc = check_feature_rows(fn, r)) return rc;
    const int64_t need = partials_bound(n_out) * a.P * 4;
    GAE_REQUIRE(n_out == 0 || !any || (workspace && workspace_bytes >= need), GAE_E_SIZE,
                "%s: workspace of %lld bytes, %lld needed (gae_embed_graphs_bwd_workspace_bytes)", fn,
                (long long)(workspace ? workspace_bytes : 0), (long long)need);
    if (!any) return GAE_OK;
    hipStream_t st = gae::as_stream(stream);
    if (n_out == 0) {                                // no graph: the gradients asked for are zeros
        for (int64_t l = 0; l < n_layers; ++l) {
            const int64_t fi = l ? widths[l - 1] : f_in, fo = widths[l];
            if (dW[l]) GAE_HIP(hipMemset2DAsync(dW[l], size_t(lddw[l]) * 4, 0, size_t(fi) * 4, size_t(fo), st));
            if (db[l]) GAE_HIP(hipMemsetAsync(db[l], 0, size_t(fo) * 4, st));
        }
        return GAE_OK;
    }
    GAE_REQUIRE(graph_ptr && d_out, GAE_E_NULL, "%s: graph_ptr / d_out is NULL", fn);
    if (const int rc = check_arrays(fn, r)) return rc;

    a.graph_ptr = graph_ptr; a.indptr = indptr; a.indices = indices; a.feat = feat; a.ldf = ldf;
    a.G = n_graphs; a.N = n_nodes; a.E = n_edges; a.B = n_out;
    a.norm_both = norm == GAE_EMBED_NORM_BOTH;
    a.graph_ids = graph_ids; a.d_out = d_out; a.ldd = ldd;
    a.part = static_cast<float *>(workspace);
    a.l_stop = a.L;
    for (int l = a.L - 1; l >= 0; --l) {
        a.W[l] = weights[l]; a.ldw[l] = ldw[l]; a.bias[l] = biases ? biases[l] : nullptr; a.act[l] = acts[l];
        a.want[l] = (dW[l] || db[l]) ? 1 : 0;
        if (a.want[l]) a.l_stop = l;
    }
    const Grid g = plan_grid(n_out, nw_max);
    a.S = g.S;
    GAE_REQUIRE(g.blocks < (int64_t(1) << 31), GAE_E_SIZE, "%s: n_out = %lld is too large", fn, (long long)n_out);
    const size_t lds = size_t(a.wfloats + g.nw * a.wave_floats) * 4;
    const char *kn = "embed_graphs_bwd_kernel";
    if (const int rc = feat_dtype == GAE_U8
                           ? gae::launch_lds<&embed_graphs_bwd_kernel<true>>(kn, g.blocks, g.nw * 64, lds, st, a)
                           : gae::launch_lds<&embed_graphs_bwd_kernel<false>>(kn, g.blocks, g.nw * 64, lds, st, a))
        return rc;
    // ---- second stage: the partials of every wave, added in the library's one order
    for (int l = 0; l < a.L; ++l) {
        if (!a.want[l]) continue;
        const int64_t fi = a.width[l], fo = a.width[l + 1];
        const gae::PartialList lw = {a.part + a.pw_off[l], dW[l], fo * fi, g.n_partials, a.P, fi, fi, lddw[l]};
        const gae::PartialList lb = {a.part + a.pb_off[l], db[l], fo, g.n_partials, a.P, fo, fo, fo};
        if (const int rc = gae::launch_partials_reduce(lw, lb, st)) return rc;
    }
    return GAE_OK;
}
