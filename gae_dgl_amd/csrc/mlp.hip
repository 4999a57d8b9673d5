// K27: a small MLP regression head trained on a frozen feature (ops.mlp, GAE.mlp_graphs, embed --mlp).
//
// d -> h1 [-> h2] -> t, ReLU on the hidden layers, squared error; 1 <= d, h <= 128, 1 <= t <= 8.  The contract -- every
// chain, the order of every elementwise step, the initialisation, the mini-batch order, the state block, the status
// block -- is the K27 comment of include/gae_hip_experimental.h; tests/mlp_ref.py restates it in numpy.
//
// Launches (ordinary ones; no grid-wide synchronisation, no atomics on floats, integer atomics on the status only):
//   check   (a fit from epoch 0 only) one thread per entry of the concatenated row list: entries of lists that no model
//           uses are skipped, row ids outside [0, n) flagged, rows that hold a non-finite value counted.
//   fit     ONE block of four waves per model, every model of the call in one grid.  The weights live in LDS for the
//           whole launch, padded with zeros to tiles of 16 (pitch in + 4 floats: rows 4 or 20 banks apart); the
//           optimiser moments stay in the model's state block in global memory (each lane owns the entries of its
//           accumulator registers: 64-byte runs).  A batch is walked in panels of 32 rows (the permuted row ids of 256 positions at a
//           time, one position per thread): gather + standardise the panel
//           into LDS, forward, output error, and per layer from the last to the first dW += Delta^T A (accumulators in
//           registers ACROSS the panels of a batch: 16 + 16 + 2 tiles of four registers per wave at most), db (one
//           thread per unit, rows in order) and dA = Delta W masked by the ReLU.  Every product is
//           v_mfma_f32_16x16x4_f32: lane l feeds A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15], the result has column
//           l & 15 and rows 4 (l >> 4) + reg.  The waves split the OUTPUT tiles of a product (column tiles w and w + 4 of a
//           32-row product, row tiles w and w + 4 of a hidden layer's dW) and never the
//           summed index, so each output element is one k-ascending fp32 fma chain.  After a batch's last panel every
//           lane applies the optimiser rule to the elements it holds.
//   predict one block per (256-row chunk, model): the same forward on panels of 32 rows.
//
// LDS: sum over the layers of outP (inP + 4) + outP weights and biases, 32 (inP + 4) activations and 32 (outP + 4) errors,
// plus 2 . 136 scaling values, 2 . 256 targets, 256 row ids and 16 words: 130 KB at 128 -> 128 -> 8, 38 KB at 48 -> 100 -> 1.
// A shape whose sum passes 160 KB (two hidden layers of 128 behind 128 features) is refused by the workspace query.
#include "common.h"
#include "feistel.h"

namespace {

using gae::cdiv;
using gae::finite32;
using gae::mfma4;
using gae::or_bits;
using gae::v4f;

constexpr int kThreads = 256, kWaves = kThreads / gae::kWave;
constexpr int kPanel = 32;                     // rows per panel: two row tiles, eight products of four rows
constexpr int kMaxWidth = 128, kMaxT = 8, kMaxModels = 4096, kMaxLists = 1024;
constexpr int kHeader = 16;                    // floats of a state block's header
constexpr int kLdsLimit = 160 * 1024;
constexpr int kIdRows = kThreads;               // batch positions whose row ids are worked out together
constexpr int kPredictRows = 256;              // rows per block of the predict launch
constexpr int kHiddenTiles = (kMaxWidth / 16) * (kMaxWidth / 16) / kWaves;     // 16 dW tiles per wave
constexpr int kOutTiles = (kMaxWidth / 16) / kWaves;                           // 2: the output layer has one row tile

struct Shape {
    int L;                                     // linear layers: 2 or 3
    int d, t;
    int in[3], out[3], inP[3], outP[3];
    int wofs[3], bofs[3];                      // offsets into a parameter set of `params` floats
    int params, state_floats;
    int lW[3], lB[3], lA[3], lD[3];            // LDS offsets in floats
    int lY, lYraw, lShift, lScale, lRid, lMisc, lds_floats;
};

__host__ __device__ inline int up16(int v) { return (v + 15) & ~15; }

__host__ __device__ inline Shape make_shape(int d, int h1, int h2, int t)
{
    Shape s;
    s.L = h2 ? 3 : 2;
    s.d = d; s.t = t;
    s.in[0] = d; s.out[0] = h1;
    if (h2) { s.in[1] = h1; s.out[1] = h2; s.in[2] = h2; s.out[2] = t; }
    else { s.in[1] = h1; s.out[1] = t; s.in[2] = 0; s.out[2] = 0; }
    int p = 0, o = 0;
    for (int l = 0; l < 3; ++l) {
        s.inP[l] = up16(s.in[l]); s.outP[l] = up16(s.out[l]);
        s.wofs[l] = p; p += s.out[l] * s.in[l];
        s.bofs[l] = p; p += s.out[l];
    }
    s.params = p;
    s.state_floats = (kHeader + 3 * p + 63) & ~63;
    for (int l = 0; l < 3; ++l) {
        const bool on = l < s.L;
        s.lW[l] = o; o += on ? s.outP[l] * (s.inP[l] + 4) : 0;
        s.lB[l] = o; o += on ? s.outP[l] : 0;
    }
    for (int l = 0; l < 3; ++l) {
        const bool on = l < s.L;
        s.lA[l] = o; o += on ? kPanel * (s.inP[l] + 4) : 0;
        s.lD[l] = o; o += on ? kPanel * (s.outP[l] + 4) : 0;
    }
    s.lY = o; o += kPanel * kMaxT;
    s.lYraw = o; o += kPanel * kMaxT;
    s.lShift = o; o += kMaxWidth + kMaxT;
    s.lScale = o; o += kMaxWidth + kMaxT;
    s.lRid = o; o += kIdRows;
    s.lMisc = o; o += 16;
    s.lds_floats = o;
    return s;
}

// The wave's tiles of a 32-row product sum_k A(m, k) B(k, n): row tiles 0 and 1 of the column tiles `wave` and `wave + 4`
// (those below ntn), continued from +0.  Element (m, k) of A at A[m am + k ak], element (k, n) of B at B[k bk + n bn], k =
// 0 .. 4 ksteps - 1 ascending.  In acc[tm][j] the lane holds column 16 (wave + 4 j) + (l & 15), rows 16 tm + 4 (l >> 4) + reg.
// Four independent chains per k step: the operands are read once for two tiles each.
__device__ __forceinline__ void pair_tiles(v4f (&acc)[2][2], const float *A, int am, int ak, const float *B, int bk, int bn,
                                           int ntn, int ksteps, int wave, int lr, int lq)
{
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    acc[0][0] = zero; acc[0][1] = zero; acc[1][0] = zero; acc[1][1] = zero;
    if (wave >= ntn) return;
    const float *pa = A + lr * am + lq * ak;
    const float *pb = B + (16 * wave + lr) * bn + lq * bk;
    const int sa = 4 * ak, sb = 4 * bk, a1 = 16 * am, b1 = 64 * bn;
    if (wave + kWaves < ntn) {
        for (int ks = 0; ks < ksteps; ++ks) {
            const float x0 = pa[ks * sa], x1 = pa[ks * sa + a1], y0 = pb[ks * sb], y1 = pb[ks * sb + b1];
            acc[0][0] = mfma4(x0, y0, acc[0][0]);
            acc[1][0] = mfma4(x1, y0, acc[1][0]);
            acc[0][1] = mfma4(x0, y1, acc[0][1]);
            acc[1][1] = mfma4(x1, y1, acc[1][1]);
        }
    } else {
        for (int ks = 0; ks < ksteps; ++ks) {
            const float x0 = pa[ks * sa], x1 = pa[ks * sa + a1], y0 = pb[ks * sb];
            acc[0][0] = mfma4(x0, y0, acc[0][0]);
            acc[1][0] = mfma4(x1, y0, acc[1][0]);
        }
    }
}

__device__ __forceinline__ float relu(float v) { return v > 0.f ? v : 0.f; }

enum { kModeTrain = 0, kModeEval = 1, kModePredict = 2 };

// The forward of one panel that stands in Act[0].  The last layer's epilogue: train: Delta = yhat - y_scaled; eval: Delta =
// (yhat / scale + shift) - y_raw; predict: out[row] = yhat / scale + shift (NaN for a row of `nanrows`).  Rows >= cnt
// and columns >= t of that Delta are zeros.  Ends with a barrier.
__device__ __forceinline__ void forward(const Shape &s, float *lds, int cnt, int mode, float *out, unsigned nanrows, int tid)
{
    const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
    for (int l = 0; l < s.L; ++l) {
        const float *A = lds + s.lA[l], *W = lds + s.lW[l], *bias = lds + s.lB[l];
        const int pA = s.inP[l] + 4, ntn = s.outP[l] / 16;
        const bool last = l == s.L - 1;
        v4f acc[2][2];
        pair_tiles(acc, A, pA, 1, W, 1, pA, ntn, s.inP[l] / 4, wave, lr, lq);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (wave + kWaves * j >= ntn) break;
            const int col = 16 * (wave + kWaves * j) + lr;
            const float b = bias[col];
#pragma unroll
            for (int tm = 0; tm < 2; ++tm) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int row = 16 * tm + 4 * lq + q;
                    const float v = acc[tm][j][q] + b;
                    if (!last) {
                        lds[s.lA[l + 1] + row * (s.outP[l] + 4) + col] = relu(v);
                    } else {
                        const bool on = row < cnt && col < s.t;
                        float r = 0.f;
                        if (on) {
                            if (mode == kModeTrain) {
                                r = v - lds[s.lY + row * kMaxT + col];
                            } else {
                                const float back = v / lds[s.lScale + s.d + col] + lds[s.lShift + s.d + col];
                                if (mode == kModeEval) r = back - lds[s.lYraw + row * kMaxT + col];
                                else out[int64_t(row) * s.t + col] = ((nanrows >> row) & 1u) ? __builtin_nanf("") : back;
                            }
                        }
                        lds[s.lD[l] + row * (s.outP[l] + 4) + col] = r;
                    }
                }
            }
        }
        __syncthreads();
    }
}

// the scaling into LDS: shift, then scale, d + t values each (NULL: 0 and 1)
__device__ __forceinline__ void load_scaling(const Shape &s, float *lds, const float *shift, const float *scale, int tid)
{
    for (int c = tid; c < s.d + s.t; c += kThreads) {
        lds[s.lShift + c] = shift ? shift[c] : 0.f;
        lds[s.lScale + c] = scale ? scale[c] : 1.f;
    }
}

// the parameters of a state block into the (zeroed) padded LDS images
__device__ __forceinline__ void load_params(const Shape &s, float *lds, const float *P, int tid)
{
    for (int l = 0; l < s.L; ++l) {
        const int in = s.in[l], pW = s.inP[l] + 4;
        for (int e = tid; e < s.out[l] * in; e += kThreads) lds[s.lW[l] + (e / in) * pW + e % in] = P[s.wofs[l] + e];
        for (int e = tid; e < s.out[l]; e += kThreads) lds[s.lB[l] + e] = P[s.bofs[l] + e];
    }
}

// ------------------------------------------------------------------------------------------------------ fit
struct FitArgs {
    const float *X, *Y;
    int64_t ldx, ldy;
    int n;
    Shape s;
    const float *shift, *scale;
    const int32_t *rows;
    int n_rows;
    const int32_t *list_ptr;
    int n_lists;
    const int32_t *train_list, *eval_list;
    const float *lr, *alpha;
    const uint64_t *seed;
    int n_models, batch;
    float beta1, beta2, eps;
    int solver;
    float momentum;
    int shuffle, final;
    int e0, e1, epochs;
    double *loss_curve, *eval_sse;
    int32_t *info;
    gae_mlp_status *status;
    float *state;
};

// [lo, hi) of list `id` when it is a list and lies inside the row list
__device__ __forceinline__ bool list_bounds(const FitArgs &a, int id, int &lo, int &hi)
{
    if (id < 0 || id >= a.n_lists) return false;
    lo = a.list_ptr[id]; hi = a.list_ptr[id + 1];
    return lo >= 0 && hi >= lo && hi <= a.n_rows;
}

__global__ __launch_bounds__(kThreads) void mlp_check_kernel(const FitArgs a)
{
    __shared__ unsigned char used[kMaxLists];
    __shared__ int bad;
    const int tid = threadIdx.x;
    for (int i = tid; i < kMaxLists; i += kThreads) used[i] = 0;
    if (tid == 0) bad = 0;
    __syncthreads();
    for (int i = tid; i < a.n_lists; i += kThreads) {
        const int lo = a.list_ptr[i], hi = a.list_ptr[i + 1];
        if (lo < 0 || hi < lo || hi > a.n_rows) bad = 1;
    }
    for (int i = tid; i < a.n_models; i += kThreads) {
        const int tl = a.train_list[i], el = a.eval_list[i];
        if (tl < 0 || tl >= a.n_lists || el < -1 || el >= a.n_lists) {
            if (blockIdx.x == 0) or_bits(&a.status->errors, GAE_MLP_ERR_LIST_ID);
        }
        if (tl >= 0 && tl < a.n_lists) used[tl] = 1;
        if (el >= 0 && el < a.n_lists) used[el] = 1;
    }
    __syncthreads();
    if (bad) {
        if (blockIdx.x == 0 && tid == 0) or_bits(&a.status->errors, GAE_MLP_ERR_LIST_PTR);
        return;
    }
    const int64_t i = int64_t(blockIdx.x) * kThreads + tid;
    if (i >= a.n_rows) return;
    bool mine = false;
    for (int k = 0; k < a.n_lists; ++k)                                // (lists may overlap: any used list that holds entry i)
        mine = mine || (used[k] && i >= a.list_ptr[k] && i < a.list_ptr[k + 1]);
    if (!mine) return;
    const int id = a.rows[i];
    if (unsigned(id) >= unsigned(a.n)) { or_bits(&a.status->errors, GAE_MLP_ERR_ROW_ID); return; }
    bool ok = true;
    for (int c = 0; c < a.s.d; ++c) ok = ok && finite32(a.X[int64_t(id) * a.ldx + c]);
    for (int c = 0; c < a.s.t; ++c) ok = ok && finite32(a.Y[int64_t(id) * a.ldy + c]);
    if (!ok) gae::add_count(&a.status->nonfinite_rows, 1);
}

using gae::feistel::shuffled;

struct Rule {
    int solver;
    float alpha, Bf, beta1, beta2, omb1, omb2, eps, step_size, bc2_sqrt, lr, momentum;
};

// one parameter: g = (chain + alpha w) / B (alpha = 0 for a bias), then the solver's rule; single fp32 operations
__device__ __forceinline__ float step_param(const Rule &r, float w, float chain, float alpha, float *gm, float *gv)
{
    const float t1 = alpha * w;
    const float t2 = chain + t1;
    const float g = t2 / r.Bf;
    if (r.solver == GAE_MLP_SGD) {
        const float a = r.momentum * *gm;
        const float b = r.lr * g;
        const float vel = a - b;
        *gm = vel;
        return w + vel;
    }
    const float ma = r.beta1 * *gm, mb = r.omb1 * g;
    const float m = ma + mb;
    const float gg = g * g;
    const float va = r.beta2 * *gv, vb = r.omb2 * gg;
    const float v = va + vb;
    *gm = m; *gv = v;
    const float sq = sqrtf(v);
    const float dn = sq / r.bc2_sqrt;
    const float den = dn + r.eps;
    const float q = m / den;
    const float u = r.step_size * q;
    return w - u;
}

// dW_l += Delta_l^T A_l over the panel's 32 rows, the chains continued in `acc`.  BY_ROWS (a hidden layer): the wave holds
// the row tiles wave and wave + 4 (output units) times every column tile (inputs), acc[8 i + tn]; else (the output layer,
// one row tile): the column tiles wave and wave + 4, acc[j].  One operand read feeds up to eight independent chains.
template <bool BY_ROWS, int MAXT>
__device__ __forceinline__ void wgrad(v4f (&acc)[MAXT], const Shape &s, const float *lds, int l, int wave, int lr, int lq)
{
    const int ntm = s.outP[l] / 16, ntn = s.inP[l] / 16, pD = s.outP[l] + 4, pA = s.inP[l] + 4;
    const float *D = lds + s.lD[l] + lq * pD + lr, *A = lds + s.lA[l] + lq * pA + lr;
    if constexpr (BY_ROWS) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int tm = wave + kWaves * i;
            if (tm >= ntm) break;
            for (int ks = 0; ks < kPanel / 4; ++ks) {
                const float x = D[4 * ks * pD + 16 * tm];
                const float *y = A + 4 * ks * pA;
#pragma unroll
                for (int tn = 0; tn < 8; ++tn)
                    if (tn < ntn) acc[8 * i + tn] = mfma4(x, y[16 * tn], acc[8 * i + tn]);
            }
        }
    } else {
        for (int ks = 0; ks < kPanel / 4; ++ks) {
            const float x = D[4 * ks * pD];
            const float *y = A + 4 * ks * pA;
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (wave + kWaves * j < ntn) acc[j] = mfma4(x, y[16 * (wave + kWaves * j)], acc[j]);
        }
    }
}

// the rule on the elements this lane's accumulators hold; the accumulators return to +0.  true: a new weight is not finite
template <bool BY_ROWS, int MAXT>
__device__ __forceinline__ bool apply(v4f (&acc)[MAXT], const Shape &s, float *lds, float *st, int l, const Rule &r, int wave,
                                      int lr, int lq)
{
    const int ntm = s.outP[l] / 16, ntn = s.inP[l] / 16, in = s.in[l], pW = s.inP[l] + 4;
    float *gm = st + kHeader + s.params + s.wofs[l], *gv = st + kHeader + 2 * s.params + s.wofs[l];
    bool bad = false;
    // the lane's corner of a tile, opaque to the optimiser: the 64 element addresses are formed where they are used and
    // not kept in registers across the epoch loop
    int row0 = 4 * lq, col0 = lr;
    asm volatile("" : "+v"(row0), "+v"(col0));
#pragma unroll
    for (int u = 0; u < MAXT; ++u) {
        const int tm = BY_ROWS ? wave + kWaves * (u / 8) : 0, tn = BY_ROWS ? u % 8 : wave + kWaves * u;
        if (tm < ntm && tn < ntn) {
            const int col = 16 * tn + col0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = 16 * tm + row0 + q;
                if (row < s.out[l] && col < in) {
                    float *w = lds + s.lW[l] + row * pW + col;
                    const float nw = step_param(r, *w, acc[u][q], r.alpha, gm + row * in + col, gv + row * in + col);
                    *w = nw;
                    bad = bad || !finite32(nw);
                }
            }
            acc[u] = v4f{0.f, 0.f, 0.f, 0.f};
        }
    }
    return bad;
}

template <int L>
__global__ __launch_bounds__(kThreads) void mlp_fit_kernel(const FitArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Shape &s = a.s;
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
    float *st = a.state + int64_t(m) * s.state_floats;
    int *misc = reinterpret_cast<int *>(lds + s.lMisc);                // [0]: a weight went non-finite; [1]: stop
    int *rid = reinterpret_cast<int *>(lds + s.lRid);
    double *loss = a.loss_curve + int64_t(m) * a.epochs;
    const double nan = __builtin_nan("");

    int lo = 0, hi = 0, info = 0;
    if (!list_bounds(a, a.train_list[m], lo, hi) || hi == lo) info = -1;        // (flagged by the check launch)
    else if (a.e0 > 0) {
        info = reinterpret_cast<const int *>(st)[6];
        if (info == 0 && reinterpret_cast<const int *>(st)[7] != a.e0) {
            info = -2;
            if (tid == 0) or_bits(&a.status->errors, GAE_MLP_ERR_RESUME);
        }
    }
    if (info != 0) {                                                   // nothing to train: the model stays as it is
        for (int e = a.e0 + tid; e < a.e1; e += kThreads) loss[e] = nan;
        if (a.final && tid < s.t) a.eval_sse[int64_t(m) * s.t + tid] = nan;
        if (tid == 0) a.info[m] = info;
        return;
    }
    const int ntr = hi - lo;
    const uint64_t seed = a.seed[m];
    int half = 1;
    while ((uint64_t(1) << (2 * half)) < uint64_t(ntr)) ++half;

    // ---- the weights: zero pads, then the state block's values or the Glorot draw
    for (int e = tid; e < s.lA[0]; e += kThreads) lds[e] = 0.f;
    if (tid < 16) misc[tid] = 0;
    load_scaling(s, lds, a.shift, a.scale, tid);
    __syncthreads();
    if (a.e0 > 0) {
        load_params(s, lds, st + kHeader, tid);
    } else {
        for (int l = 0; l < s.L; ++l) {
            const int in = s.in[l], pW = s.inP[l] + 4;
            const float bound = float(sqrt(6.0 / double(s.in[l] + s.out[l])));
            for (int e = tid; e < s.out[l] * (in + 1); e += kThreads) {
                const bool isb = e >= s.out[l] * in;
                const int k = isb ? e - s.out[l] * in : e;
                uint32_t c[4];
                gae::philox4x32_10(uint64_t(k) >> 2, uint64_t(2 * l + (isb ? 1 : 0)), seed, c);
                const float u = float(c[k & 3] >> 8) * (1.0f / 16777216.0f);
                const float two_u = 2.0f * u;
                const float centred = two_u - 1.0f;
                const float w = centred * bound;
                if (isb) lds[s.lB[l] + k] = w;
                else lds[s.lW[l] + (k / in) * pW + k % in] = w;
            }
        }
        for (int e = tid; e < 2 * s.params; e += kThreads) st[kHeader + s.params + e] = 0.f;
        for (int e = kHeader + 3 * s.params + tid; e < s.state_floats; e += kThreads) st[e] = 0.f;      // the block's tail
        if (tid >= 8 && tid < kHeader) st[tid] = 0.f;                                                  // reserved
    }
    int64_t step = a.e0 > 0 ? reinterpret_cast<const int64_t *>(st)[0] : 0;
    double b1p = a.e0 > 0 ? reinterpret_cast<const double *>(st)[1] : 1.0;
    double b2p = a.e0 > 0 ? reinterpret_cast<const double *>(st)[2] : 1.0;
    __syncthreads();

    v4f acc0[kHiddenTiles], acc1[L == 3 ? kHiddenTiles : 8], accO[kOutTiles];
#pragma unroll
    for (int u = 0; u < kHiddenTiles; ++u) acc0[u] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < (L == 3 ? kHiddenTiles : 8); ++u) acc1[u] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < kOutTiles; ++u) accO[u] = v4f{0.f, 0.f, 0.f, 0.f};
    float db[3] = {0.f, 0.f, 0.f};

    Rule r;
    r.solver = a.solver; r.alpha = a.alpha[m]; r.lr = a.lr[m]; r.momentum = a.momentum;
    r.beta1 = a.beta1; r.beta2 = a.beta2; r.omb1 = 1.0f - a.beta1; r.omb2 = 1.0f - a.beta2; r.eps = a.eps;
    r.Bf = 1.f; r.step_size = 0.f; r.bc2_sqrt = 1.f;

    int stopped = 0;
    for (int ep = a.e0; ep < a.e1 && !stopped; ++ep) {
        double sse = 0.0;
        for (int b0 = 0; b0 < ntr; b0 += a.batch) {
            const int B = ntr - b0 < a.batch ? ntr - b0 : a.batch;
            for (int r0 = 0; r0 < B; r0 += kPanel) {
                const int cnt = B - r0 < kPanel ? B - r0 : kPanel;
                // the row ids of the next kIdRows positions of the batch, one position per thread: the keyed permutation
                // costs some forty Philox blocks per position, far more than a panel's products on one wave
                if (r0 % kIdRows == 0) {
                    int id = -1;
                    if (r0 + tid < B) {
                        const uint32_t p = uint32_t(b0 + r0 + tid);
                        const uint32_t q = a.shuffle ? shuffled(p, uint32_t(ntr), half, seed, uint32_t(ep)) : p;
                        id = a.rows[lo + int(q)];
                        if (unsigned(id) >= unsigned(a.n)) id = -1;            // (flagged by the check launch): a zero row
                    }
                    rid[tid] = id;
                }
                const int *pid = rid + r0 % kIdRows;                           // (-1 past the batch's end)
                __syncthreads();
                {
                    float *X0 = lds + s.lA[0];
                    const int w0 = s.inP[0], p0 = w0 + 4;
                    for (int e = tid; e < kPanel * w0; e += kThreads) {
                        const int i = e / w0, c = e % w0, id = pid[i];
                        float v = 0.f;
                        if (id >= 0 && c < s.d) {
                            const float centred = a.X[int64_t(id) * a.ldx + c] - lds[s.lShift + c];
                            v = centred * lds[s.lScale + c];
                        }
                        X0[i * p0 + c] = v;
                    }
                    for (int e = tid; e < kPanel * s.t; e += kThreads) {
                        const int i = e / s.t, c = e % s.t, id = pid[i];
                        float v = 0.f;
                        if (id >= 0) {
                            const float centred = a.Y[int64_t(id) * a.ldy + c] - lds[s.lShift + s.d + c];
                            v = centred * lds[s.lScale + s.d + c];
                        }
                        lds[s.lY + i * kMaxT + c] = v;
                    }
                }
                __syncthreads();
                forward(s, lds, cnt, kModeTrain, nullptr, 0u, tid);
                if (tid == 0) {
                    const float *D = lds + s.lD[L - 1];
                    const int pD = s.outP[L - 1] + 4;
                    for (int i = 0; i < cnt; ++i)
                        for (int j = 0; j < s.t; ++j) {
                            const double e = double(D[i * pD + j]);
                            const double e2 = e * e;
                            sse = sse + e2;
                        }
                }
#pragma unroll
                for (int l = L - 1; l >= 0; --l) {
                    if (l == L - 1) wgrad<false>(accO, s, lds, l, wave, lr, lq);
                    else if (l == 0) wgrad<true>(acc0, s, lds, l, wave, lr, lq);
                    else wgrad<true>(acc1, s, lds, l, wave, lr, lq);
                    const int pD = s.outP[l] + 4;
                    const float *D = lds + s.lD[l];
                    if (tid < s.out[l]) {
                        float g = db[l];
                        for (int i = 0; i < kPanel; ++i) g = g + D[i * pD + tid];
                        db[l] = g;
                    }
                    if (l > 0) {
                        const int ntn = s.inP[l] / 16, pP = s.inP[l] + 4;
                        const float *W = lds + s.lW[l], *H = lds + s.lA[l];
                        float *Dp = lds + s.lD[l - 1];
                        v4f g[2][2];
                        pair_tiles(g, D, pD, 1, W, pP, 1, ntn, s.outP[l] / 4, wave, lr, lq);
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            if (wave + kWaves * j >= ntn) break;
#pragma unroll
                            for (int tm = 0; tm < 2; ++tm) {
#pragma unroll
                                for (int q = 0; q < 4; ++q) {
                                    const int at = (16 * tm + 4 * lq + q) * pP + 16 * (wave + kWaves * j) + lr;
                                    Dp[at] = H[at] > 0.f ? g[tm][j][q] : 0.f;
                                }
                            }
                        }
                        __syncthreads();
                    }
                }
            }
            // ---- the batch's step
            step += 1;
            b1p = b1p * double(a.beta1);
            b2p = b2p * double(a.beta2);
            r.Bf = float(B);
            r.step_size = float(double(r.lr) / (1.0 - b1p));
            r.bc2_sqrt = float(sqrt(1.0 - b2p));
            bool bad = false;
#pragma unroll
            for (int l = 0; l < L; ++l) {
                if (l == L - 1) bad = apply<false>(accO, s, lds, st, l, r, wave, lr, lq) || bad;
                else if (l == 0) bad = apply<true>(acc0, s, lds, st, l, r, wave, lr, lq) || bad;
                else bad = apply<true>(acc1, s, lds, st, l, r, wave, lr, lq) || bad;
                if (tid < s.out[l]) {
                    float *bl = lds + s.lB[l] + tid;
                    const float nb = step_param(r, *bl, db[l], 0.f, st + kHeader + s.params + s.bofs[l] + tid,
                                                st + kHeader + 2 * s.params + s.bofs[l] + tid);
                    *bl = nb;
                    bad = bad || !finite32(nb);
                }
                db[l] = 0.f;
            }
            if (bad) misc[0] = 1;
        }
        __syncthreads();
        if (tid == 0) {
            const double twice = 2.0 * double(ntr);
            const double value = sse / twice;
            loss[ep] = value;
            const bool fin = gae::finite64(value);
            misc[1] = (misc[0] || !fin) ? 1 : 0;
        }
        __syncthreads();
        if (misc[1]) {
            stopped = 1;
            info = 1 + ep;
            for (int e = ep + 1 + tid; e < a.e1; e += kThreads) loss[e] = nan;
        }
    }

    // ---- the state block
    for (int l = 0; l < s.L; ++l) {
        const int in = s.in[l], pW = s.inP[l] + 4;
        for (int e = tid; e < s.out[l] * in; e += kThreads) st[kHeader + s.wofs[l] + e] = lds[s.lW[l] + (e / in) * pW + e % in];
        for (int e = tid; e < s.out[l]; e += kThreads) st[kHeader + s.bofs[l] + e] = lds[s.lB[l] + e];
    }
    if (tid == 0) {
        reinterpret_cast<int64_t *>(st)[0] = step;
        reinterpret_cast<double *>(st)[1] = b1p;
        reinterpret_cast<double *>(st)[2] = b2p;
        reinterpret_cast<int *>(st)[6] = info;
        reinterpret_cast<int *>(st)[7] = a.e1;
        a.info[m] = info;
    }
    if (!a.final) return;

    // ---- the held-out squared error, in the targets' own units, rows in list order
    int elo = 0, ehi = 0;
    const int el = a.eval_list[m];
    if (info != 0 || el < 0 || !list_bounds(a, el, elo, ehi)) {
        if (tid < s.t) a.eval_sse[int64_t(m) * s.t + tid] = nan;
        return;
    }
    double esse = 0.0;
    for (int r0 = elo; r0 < ehi; r0 += kPanel) {
        const int cnt = ehi - r0 < kPanel ? ehi - r0 : kPanel;
        __syncthreads();
        if (tid < kPanel) {
            int id = tid < cnt ? a.rows[r0 + tid] : -1;
            if (unsigned(id) >= unsigned(a.n)) id = -1;
            rid[tid] = id;
        }
        __syncthreads();
        float *X0 = lds + s.lA[0];
        const int w0 = s.inP[0], p0 = w0 + 4;
        for (int e = tid; e < kPanel * w0; e += kThreads) {
            const int i = e / w0, c = e % w0, id = rid[i];
            float v = 0.f;
            if (id >= 0 && c < s.d) {
                const float centred = a.X[int64_t(id) * a.ldx + c] - lds[s.lShift + c];
                v = centred * lds[s.lScale + c];
            }
            X0[i * p0 + c] = v;
        }
        for (int e = tid; e < kPanel * s.t; e += kThreads) {
            const int i = e / s.t, c = e % s.t, id = rid[i];
            lds[s.lYraw + i * kMaxT + c] = id >= 0 ? a.Y[int64_t(id) * a.ldy + c] : 0.f;
        }
        __syncthreads();
        forward(s, lds, cnt, kModeEval, nullptr, 0u, tid);
        if (tid < s.t) {
            const float *D = lds + s.lD[L - 1];
            const int pD = s.outP[L - 1] + 4;
            for (int i = 0; i < cnt; ++i) {
                const double e = double(D[i * pD + tid]);
                const double e2 = e * e;
                esse = esse + e2;
            }
        }
    }
    if (tid < s.t) a.eval_sse[int64_t(m) * s.t + tid] = esse;
}

// ------------------------------------------------------------------------------------------------------ predict
struct PredictArgs {
    const float *X;
    int64_t ldx;
    int n;
    Shape s;
    const float *shift, *scale;
    const float *state;
    float *out;
    gae_mlp_status *status;
};

__global__ __launch_bounds__(kThreads) void mlp_predict_kernel(const PredictArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Shape &s = a.s;
    const int m = blockIdx.y, tid = threadIdx.x;
    unsigned *misc = reinterpret_cast<unsigned *>(lds + s.lMisc);      // [0]: the panel's rows that hold a non-finite feature
    for (int e = tid; e < s.lA[0]; e += kThreads) lds[e] = 0.f;
    if (tid < 16) misc[tid] = 0u;
    load_scaling(s, lds, a.shift, a.scale, tid);
    __syncthreads();
    load_params(s, lds, a.state + int64_t(m) * s.state_floats + kHeader, tid);
    const int64_t first = int64_t(blockIdx.x) * kPredictRows;
    const int64_t end = first + kPredictRows < a.n ? first + kPredictRows : a.n;
    unsigned counted = 0;
    for (int64_t r0 = first; r0 < end; r0 += kPanel) {
        const int cnt = end - r0 < kPanel ? int(end - r0) : kPanel;
        __syncthreads();
        if (tid == 0) misc[0] = 0u;
        __syncthreads();
        float *X0 = lds + s.lA[0];
        const int w0 = s.inP[0], p0 = w0 + 4;
        for (int e = tid; e < kPanel * w0; e += kThreads) {
            const int i = e / w0, c = e % w0;
            float v = 0.f;
            if (i < cnt && c < s.d) {
                const float x = a.X[(r0 + i) * a.ldx + c];
                if (!finite32(x)) atomicOr(&misc[0], 1u << i);
                const float centred = x - lds[s.lShift + c];
                v = centred * lds[s.lScale + c];
            }
            X0[i * p0 + c] = v;
        }
        __syncthreads();
        const unsigned nanrows = misc[0];
        forward(s, lds, cnt, kModePredict, a.out + (int64_t(m) * a.n + r0) * s.t, nanrows, tid);
        counted += __popc(nanrows);
    }
    if (m == 0 && tid == 0 && counted && a.status)
        gae::add_count(&a.status->nonfinite_rows, counted);
}

// the workspace: n_models state blocks, one after another
float *carve(gae::Carver &c, const Shape &s, int64_t n_models) { return c.take<float>(n_models * int64_t(s.state_floats)); }

// the shape checks every entry point shares; `need`: the workspace's bytes
int plan(const char *fn, int64_t d, int64_t h1, int64_t h2, int64_t t, int64_t n_models, Shape &s, int64_t &need)
{
    GAE_REQUIRE(d >= 1 && d <= kMaxWidth, GAE_E_RANGE, "%s: d = %lld outside 1..128", fn, (long long)d);
    GAE_REQUIRE(h1 >= 1 && h1 <= kMaxWidth, GAE_E_RANGE, "%s: h1 = %lld outside 1..128", fn, (long long)h1);
    GAE_REQUIRE(h2 >= 0 && h2 <= kMaxWidth, GAE_E_RANGE, "%s: h2 = %lld outside 0..128 (0: one hidden layer)", fn,
                (long long)h2);
    GAE_REQUIRE(t >= 1 && t <= kMaxT, GAE_E_RANGE, "%s: t = %lld outside 1..8", fn, (long long)t);
    GAE_REQUIRE(n_models >= 1 && n_models <= kMaxModels, GAE_E_RANGE, "%s: n_models = %lld outside 1..4096", fn,
                (long long)n_models);
    s = make_shape(int(d), int(h1), int(h2), int(t));
    GAE_REQUIRE(int64_t(s.lds_floats) * 4 <= kLdsLimit, GAE_E_RANGE,
                "%s: %lld -> %lld -> %lld -> %lld needs %lld bytes of LDS, a block has %d", fn, (long long)d, (long long)h1,
                (long long)h2, (long long)t, (long long)s.lds_floats * 4, kLdsLimit);
    gae::Carver c(nullptr);
    carve(c, s, n_models);
    need = c.bytes();
    return GAE_OK;
}

} // namespace

extern "C" int64_t gae_mlp_workspace_bytes(int64_t d, int64_t h1, int64_t h2, int64_t t, int64_t n_models)
{
    Shape s;
    int64_t need = 0;
    if (const int rc = plan("gae_mlp_workspace_bytes", d, h1, h2, t, n_models, s, need)) return rc;
    return need;
}

extern "C" int gae_mlp_fit(const float *X, int64_t ldx, const float *Y, int64_t ldy, int64_t n, int64_t d, int64_t h1,
                           int64_t h2, int64_t t, const float *shift, const float *scale, const int32_t *rows,
                           int64_t n_rows, const int32_t *list_ptr, int64_t n_lists, const int32_t *train_list,
                           const int32_t *eval_list, const float *lr, const float *alpha, const uint64_t *seed,
                           int64_t n_models, int64_t batch_size, float beta1, float beta2, float eps, int solver,
                           float momentum, int flags, int64_t e0, int64_t e1, int64_t epochs, double *loss_curve,
                           double *eval_sse, int32_t *info, gae_mlp_status *status, void *workspace,
                           int64_t workspace_bytes, void *stream)
{
    const char *fn = "gae_mlp_fit";
    FitArgs a;
    int64_t need = 0;
    if (const int rc = plan(fn, d, h1, h2, t, n_models, a.s, need)) return rc;
    GAE_REQUIRE(n >= 0 && n < (int64_t(1) << 31), GAE_E_SIZE, "%s: n = %lld outside 0..2^31 - 1", fn, (long long)n);
    GAE_REQUIRE(n_rows >= 1 && n_rows < (int64_t(1) << 31), GAE_E_SIZE, "%s: n_rows = %lld outside 1..2^31 - 1", fn,
                (long long)n_rows);
    GAE_REQUIRE(n_lists >= 1 && n_lists <= kMaxLists, GAE_E_RANGE, "%s: n_lists = %lld outside 1..1024", fn,
                (long long)n_lists);
    GAE_REQUIRE(ldx >= d && ldy >= t, GAE_E_SIZE, "%s: leading dimension too small (ldx %lld < d or ldy %lld < t)", fn,
                (long long)ldx, (long long)ldy);
    GAE_REQUIRE(batch_size >= 1 && batch_size < (int64_t(1) << 31), GAE_E_RANGE, "%s: batch_size = %lld outside 1..2^31 - 1",
                fn, (long long)batch_size);
    GAE_REQUIRE(solver == GAE_MLP_ADAM || solver == GAE_MLP_SGD, GAE_E_RANGE, "%s: unknown solver %d", fn, solver);
    GAE_REQUIRE((flags & ~(GAE_MLP_SHUFFLE | GAE_MLP_FINAL)) == 0, GAE_E_RANGE, "%s: unknown flags 0x%x", fn, flags);
    GAE_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps > 0.f && momentum >= 0.f && momentum < 1.f,
                GAE_E_RANGE, "%s: beta1 = %g, beta2 = %g, momentum = %g outside [0, 1) or eps = %g <= 0", fn, beta1, beta2,
                momentum, eps);
    GAE_REQUIRE(epochs >= 1 && epochs < (int64_t(1) << 31) && e0 >= 0 && e0 < e1 && e1 <= epochs, GAE_E_RANGE,
                "%s: epochs [%lld, %lld) of %lld", fn, (long long)e0, (long long)e1, (long long)epochs);
    GAE_REQUIRE(X && Y && rows && list_ptr && train_list && eval_list && lr && alpha && seed, GAE_E_NULL,
                "%s: X / Y / rows / list_ptr / train_list / eval_list / lr / alpha / seed is NULL", fn);
    GAE_REQUIRE(loss_curve && eval_sse && info && status, GAE_E_NULL, "%s: loss_curve / eval_sse / info / status is NULL", fn);
    GAE_REQUIRE(workspace, GAE_E_NULL, "%s: workspace is NULL", fn);
    GAE_REQUIRE(workspace_bytes >= need, GAE_E_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn,
                (long long)workspace_bytes, (long long)need);

    gae::Carver c(workspace);
    a.state = carve(c, a.s, n_models);
    a.X = X; a.Y = Y; a.ldx = ldx; a.ldy = ldy; a.n = int(n);
    a.shift = shift; a.scale = scale; a.rows = rows; a.n_rows = int(n_rows); a.list_ptr = list_ptr; a.n_lists = int(n_lists);
    a.train_list = train_list; a.eval_list = eval_list; a.lr = lr; a.alpha = alpha; a.seed = seed;
    a.n_models = int(n_models); a.batch = int(batch_size);
    a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.solver = solver; a.momentum = momentum;
    a.shuffle = (flags & GAE_MLP_SHUFFLE) ? 1 : 0; a.final = (flags & GAE_MLP_FINAL) ? 1 : 0;
    a.e0 = int(e0); a.e1 = int(e1); a.epochs = int(epochs);
    a.loss_curve = loss_curve; a.eval_sse = eval_sse; a.info = info; a.status = status;
    hipStream_t st = gae::as_stream(stream);
    if (e0 == 0) {
        hipLaunchKernelGGL(mlp_check_kernel, dim3(unsigned(cdiv(n_rows, kThreads))), dim3(kThreads), 0, st, a);
        GAE_CHECK_LAUNCH("mlp_check_kernel");
    }
    const size_t lds = size_t(a.s.lds_floats) * 4;
    if (a.s.L == 3) return gae::launch_lds<&mlp_fit_kernel<3>>("mlp_fit_kernel", n_models, kThreads, lds, st, a);
    return gae::launch_lds<&mlp_fit_kernel<2>>("mlp_fit_kernel", n_models, kThreads, lds, st, a);
}

extern "C" int gae_mlp_predict(const float *X, int64_t ldx, int64_t n, int64_t d, int64_t h1, int64_t h2, int64_t t,
                               const float *shift, const float *scale, const void *state, int64_t n_models, float *out,
                               gae_mlp_status *status, void *stream)
{
    const char *fn = "gae_mlp_predict";
    PredictArgs a;
    int64_t need = 0;
    if (const int rc = plan(fn, d, h1, h2, t, n_models, a.s, need)) return rc;
    GAE_REQUIRE(n >= 0 && n < (int64_t(1) << 31), GAE_E_SIZE, "%s: n = %lld outside 0..2^31 - 1", fn, (long long)n);
    GAE_REQUIRE(ldx >= d, GAE_E_SIZE, "%s: ldx = %lld < d", fn, (long long)ldx);
    GAE_REQUIRE(state, GAE_E_NULL, "%s: state is NULL", fn);
    GAE_REQUIRE(n == 0 || (X && out), GAE_E_NULL, "%s: X / out is NULL", fn);
    if (n == 0) return GAE_OK;
    a.X = X; a.ldx = ldx; a.n = int(n); a.shift = shift; a.scale = scale;
    a.state = static_cast<const float *>(state); a.out = out; a.status = status;
    static int configured[16] = {0};
    const size_t lds = size_t(a.s.lds_floats) * 4;
    int dev = 0;
    GAE_HIP(hipGetDevice(&dev));
    if (lds > 48 * 1024 && (dev < 0 || dev >= 16 || configured[dev] < int(lds))) {
        GAE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(mlp_predict_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
        if (dev >= 0 && dev < 16) configured[dev] = int(lds);
    }
    hipLaunchKernelGGL(mlp_predict_kernel, dim3(unsigned(cdiv(n, kPredictRows)), unsigned(n_models)), dim3(kThreads), lds,
                       gae::as_stream(stream), a);
    GAE_CHECK_LAUNCH("mlp_predict_kernel");
    return GAE_OK;
}
