// K37 / K38: the DeepWalk baseline (ops.random_walks, ops.sgns_train, ops.deepwalk): uniform first-order random walks
// over a CSR as stored, and a SYNCHRONOUS mini-batch skip-gram trainer with negatives shared per walk and element-wise
// Adagrad.  It is not a port of word2vec's asynchronous loop: that one is order-dependent, this one gives the same bits run
// to run and equals the numpy restatement (tests/deepwalk_ref.py) bit for bit.
//
// THE CONTRACT is the K37 / K38 comment of include/gae_hip_experimental.h: the Philox words of every step and of every
// negative, the positives of a walk, every fp32 fma chain and its order, the coefficient formulas, the fixed-point scatter
// and the Adagrad sequence.
//
// Launches (ordinary ones; no float atomic anywhere, 64-bit integer atomics on the accumulators and the status):
//   walks       one thread per walk, a latency-bound pointer chase: one Philox block per four steps, integers only.
//   init        one thread per element of W: K27's uniform draw.
//   order       one thread per position of the epoch: the Feistel permutation of feistel.h.
//   accumulate  ONE block of four waves per walk of the batch.  The walk's rows of W and of C and the M negative rows of C
//               stand in LDS, padded with zeros to tiles of 16 (pitch + 4 floats).  Every product is
//               v_mfma_f32_16x16x4_f32; the waves split the OUTPUT tiles of a product (tile t of a product goes to wave
//               t mod 4) and never the summed index, so each output element is one ascending fp32 fma chain.  The logit
//               tiles are turned into coefficients in their epilogue (fp64 sigma of sigma64.h), the gradient tiles are
//               scattered from their registers: x -> llrint(x 2^32), one 64-bit integer add each.
//   update      one grid-stride sweep over both tables: Adagrad on the elements whose accumulator is not zero.
//
// LDS of accumulate: (2 LP + M) (dP + 4) row floats + LP (LP + M + 4) coefficients + 64 + 128 words, LP = L up to 16, dP = d
// up to 16: 44 288 bytes at L = 40, d = 64, M = 16 and 135 936 bytes at L = 64, d = 128, M = 64.
//
// SAFETY: a walk-table entry outside [-1, n) is flagged and read as -1; an order entry outside [0, n_walks) is flagged and
// its block returns; a bad row pointer reads as a sink, a bad column or start ends the walk; the noise search is bounded
// and returns an index of [0, n) whatever the table holds.
#include "common.h"
#include "feistel.h"
#include "sigma64.h"

namespace {

using gae::cdiv;
using gae::mfma4;
using gae::or_bits;
using gae::v4f;

constexpr int kThreads = 256, kWaves = kThreads / gae::kWave;
constexpr int kMaxWalkLength = GAE_DEEPWALK_MAX_LENGTH;
constexpr int kMaxL = GAE_SGNS_MAX_LENGTH, kMaxD = GAE_SGNS_MAX_DIM, kMaxK = GAE_SGNS_MAX_NEGATIVES;
constexpr int64_t kMaxGrid = int64_t(1) << 20;           // blocks of a grid-stride sweep

__host__ __device__ inline int up16(int v) { return (v + 15) & ~15; }

// ------------------------------------------------------------------------------------------------------ K37: walks
struct WalkArgs {
    const int64_t *indptr;
    const int32_t *indices;
    int64_t n, nnz;
    const int32_t *starts;
    int64_t m, n_walks;
    int L;
    uint64_t seed;
    int32_t *walks;
    int64_t *status;
};

__global__ __launch_bounds__(kThreads) void random_walks_kernel(const WalkArgs a)
{
    const int64_t w = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (w >= a.n_walks) return;
    const int64_t s = w % a.m;
    int32_t *out = a.walks + w * a.L;
    int64_t bits = 0;
    int64_t v = a.starts ? int64_t(a.starts[s]) : s;
    if (v < 0 || v >= a.n) { bits |= GAE_DEEPWALK_ERR_START; v = -1; }
    out[0] = int32_t(v);
    uint32_t c[4] = {0u, 0u, 0u, 0u};
    for (int t = 1; t < a.L; ++t) {
        if (v >= 0) {
            if (t == 1 || (t & 3) == 0) gae::philox4x32_10(uint64_t(w), GAE_DEEPWALK_WALK_DRAW + uint64_t(t >> 2), a.seed, c);
            const int64_t b = a.indptr[v], e = a.indptr[v + 1];
            int64_t deg = e - b;
            if (b < 0 || e < b || e > a.nnz || deg > int64_t(0xFFFFFFFFll)) { bits |= GAE_DEEPWALK_ERR_INDPTR; deg = 0; }
            if (deg == 0) {
                v = -1;
            } else {
                const int64_t col = a.indices[b + int64_t((uint64_t(c[t & 3]) * uint64_t(deg)) >> 32)];
                if (col < 0 || col >= a.n) { bits |= GAE_DEEPWALK_ERR_COLUMN; v = -1; }
                else v = col;
            }
        }
        out[t] = int32_t(v);
    }
    if (bits) or_bits(a.status, bits);
}

// ------------------------------------------------------------------------------------------------------ K38: init, order
__global__ __launch_bounds__(kThreads) void sgns_init_kernel(float *W, int64_t count, uint64_t seed, float bound)
{
    for (int64_t e = int64_t(blockIdx.x) * kThreads + threadIdx.x; e < count; e += int64_t(gridDim.x) * kThreads) {
        uint32_t c[4];
        gae::philox4x32_10(uint64_t(e) >> 2, GAE_SGNS_INIT_DRAW, seed, c);
        const float u = float(c[e & 3] >> 8) * (1.0f / 16777216.0f);
        const float two_u = 2.0f * u;
        const float centred = two_u - 1.0f;
        W[e] = centred * bound;
    }
}

__global__ __launch_bounds__(kThreads) void sgns_order_kernel(int32_t *order, uint32_t n_walks, int half, uint64_t seed,
                                                              uint32_t epoch)
{
    const int64_t p = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (p < n_walks) order[p] = int32_t(gae::feistel::shuffled(uint32_t(p), n_walks, half, seed, epoch));
}

// ------------------------------------------------------------------------------------------------------ K38: accumulate
struct SgnsArgs {
    const int32_t *walks, *order;
    int64_t n_walks, first;
    int L, LP, d, dP, M, window, K;
    const int64_t *cum;
    int64_t n;
    uint64_t seed;
    uint32_t epoch;
    const float *W, *C;
    int64_t *AW, *AC, *status;
};

// LDS offsets in floats: the walk's rows of W, the rows of C (contexts, then negatives), the coefficients [LP, LP + M], the
// negatives' weight per row, the node of every row of the C block
struct Layout { int pd, pg, ww, cc, g, coef, cid, floats; };

__host__ __device__ inline Layout make_layout(int LP, int dP, int M)
{
    Layout l;
    l.pd = dP + 4; l.pg = LP + M + 4;
    l.ww = 0;
    l.cc = l.ww + LP * l.pd;
    l.g = l.cc + (LP + M) * l.pd;
    l.coef = l.g + LP * l.pg;
    l.cid = l.coef + kMaxL;
    l.floats = l.cid + 2 * kMaxL;
    return l;
}

// the node drawn by a 64-bit word: the largest i of [0, n) with cum[i] <= umul64hi(u, cum[n]); -1 on an empty table
__device__ __forceinline__ int noise_node(const int64_t *cum, int64_t n, uint64_t u)
{
    const int64_t total = cum[n];
    if (total <= 0) return -1;
    const int64_t target = int64_t(__umul64hi(u, uint64_t(total)));
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (cum[mid] <= target) lo = mid; else hi = mid;
    }
    return int(lo);
}

// one gradient element into its fixed-point accumulator; true: outside the frame (not added)
__device__ __forceinline__ bool scatter(int64_t *acc, float x)
{
    if (!(fabsf(x) < 1048576.0f)) return true;
    const long long v = __double2ll_rn(double(x) * 4294967296.0);
    if (v != 0) atomicAdd(reinterpret_cast<unsigned long long *>(acc), static_cast<unsigned long long>(v));
    return false;
}

__global__ __launch_bounds__(kThreads) void sgns_accumulate_kernel(const SgnsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int L = a.L, LP = a.LP, d = a.d, dP = a.dP, M = a.M;
    const Layout lay = make_layout(LP, dP, M);
    const int pd = lay.pd, pg = lay.pg;
    float *Ww = lds + lay.ww, *Cc = lds + lay.cc, *G = lds + lay.g, *coef = lds + lay.coef;
    int *cid = reinterpret_cast<int *>(lds + lay.cid);

    const int64_t wid = a.order[a.first + blockIdx.x];
    if (wid < 0 || wid >= a.n_walks) {                                 // (uniform over the block)
        if (tid == 0) or_bits(a.status, GAE_DEEPWALK_ERR_ORDER);
        return;
    }

    // ---- the nodes: the walk's positions, then the M negatives of this (epoch, walk)
    if (tid < LP + M) {
        int id = -1;
        if (tid < LP) {
            if (tid < L) {
                id = a.walks[wid * L + tid];
                if (id < -1 || id >= a.n) { or_bits(a.status, GAE_DEEPWALK_ERR_NODE); id = -1; }
            }
        } else {
            const int slot = tid - LP;
            uint32_t c[4];
            gae::philox4x32_10((uint64_t(a.epoch) << 32) | uint64_t(wid), GAE_SGNS_NEG_DRAW + uint64_t(slot >> 1), a.seed, c);
            const uint64_t u = (uint64_t(c[2 * (slot & 1) + 1]) << 32) | c[2 * (slot & 1)];
            id = noise_node(a.cum, a.n, u);
        }
        cid[tid] = id;
    }
    __syncthreads();

    // ---- the negatives' weight of every row, and the rows themselves (an invalid or padded position: a row of +0)
    if (tid < LP) {
        int c = 0;
        if (cid[tid] >= 0) {
            const int j0 = tid - a.window > 0 ? tid - a.window : 0, j1 = tid + a.window < L - 1 ? tid + a.window : L - 1;
            for (int j = j0; j <= j1; ++j) c += (j != tid && cid[j] >= 0) ? 1 : 0;
        }
        coef[tid] = float(a.K * c) / float(M);
    }
    for (int e = tid; e < (2 * LP + M) * dP; e += kThreads) {
        const int r = e / dP, f = e - r * dP;
        const bool is_w = r < LP;
        const int id = cid[is_w ? r : r - LP];
        float v = 0.f;
        if (id >= 0 && f < d) v = (is_w ? a.W : a.C)[int64_t(id) * d + f];
        (is_w ? Ww + r * pd : Cc + (r - LP) * pd)[f] = v;
    }
    __syncthreads();

    // ---- logits -> coefficients: tile (tm, tn) of [S | N] = Ww [Cw | Cn]^T, the chain over the feature index
    const int ntm = LP / 16, ntn = (LP + M) / 16, ntf = dP / 16;
    for (int t = wave; t < ntm * ntn; t += kWaves) {
        const int tm = t / ntn, tn = t - tm * ntn;
        const float *pa = Ww + (16 * tm + lr) * pd + lq, *pb = Cc + (16 * tn + lr) * pd + lq;
        v4f acc = {0.f, 0.f, 0.f, 0.f};
        for (int ks = 0; ks < dP / 4; ++ks) acc = mfma4(pa[4 * ks], pb[4 * ks], acc);
        const int col = 16 * tn + lr, cnode = cid[col];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int p = 16 * tm + 4 * lq + q, pnode = cid[p];
            float g = 0.f;
            if (col < LP) {
                const int dist = p > col ? p - col : col - p;
                if (pnode >= 0 && cnode >= 0 && dist > 0 && dist <= a.window)
                    g = float(gae::sigma64::sigma(-double(acc[q])));
            } else if (pnode >= 0 && cnode >= 0 && cnode != pnode) {
                const float s = float(gae::sigma64::sigma(double(acc[q])));
                const float cs = coef[p] * s;
                g = -cs;
            }
            G[p * pg + col] = g;
        }
    }
    __syncthreads();

    // ---- gradients, scattered from the registers: dW = G [Cw ; Cn] (chain over contexts, then negatives) and
    //      [dCw ; dCn] = G^T Ww (chain over the walk's positions)
    bool bad = false;
    const int t_w = ntm * ntf, t_all = t_w + ntn * ntf;
    for (int t = wave; t < t_all; t += kWaves) {
        const bool is_w = t < t_w;
        const int u = is_w ? t : t - t_w;
        const int tr = u / ntf, tf = u - tr * ntf;
        v4f acc = {0.f, 0.f, 0.f, 0.f};
        if (is_w) {
            const float *pa = G + (16 * tr + lr) * pg + lq, *pb = Cc + lq * pd + 16 * tf + lr;
            for (int ks = 0; ks < (LP + M) / 4; ++ks) acc = mfma4(pa[4 * ks], pb[4 * ks * pd], acc);
        } else {
            const float *pa = G + lq * pg + 16 * tr + lr, *pb = Ww + lq * pd + 16 * tf + lr;
            for (int ks = 0; ks < LP / 4; ++ks) acc = mfma4(pa[4 * ks * pg], pb[4 * ks * pd], acc);
        }
        const int f = 16 * tf + lr;
        int64_t *A = is_w ? a.AW : a.AC;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int id = cid[16 * tr + 4 * lq + q];
            if (id >= 0 && f < d) bad = scatter(A + int64_t(id) * d + f, acc[q]) || bad;
        }
    }
    if (bad) or_bits(a.status, GAE_DEEPWALK_ERR_RANGE);
}

// ------------------------------------------------------------------------------------------------------ K38: update
struct UpdateArgs {
    float *X[2], *H[2];
    int64_t *A[2];
    int64_t count;                         // elements of one table
    float lr, eps;
    int64_t *status;
};

__global__ __launch_bounds__(kThreads) void sgns_update_kernel(const UpdateArgs a)
{
    bool bad = false;
    for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < 2 * a.count; i += int64_t(gridDim.x) * kThreads) {
        const int tb = i >= a.count ? 1 : 0;
        const int64_t e = i - (tb ? a.count : 0);
        const int64_t acc = a.A[tb][e];
        if (acc == 0) continue;
        const float g = float(double(acc) * (1.0 / 4294967296.0));
        const float h = fmaf(g, g, a.H[tb][e]);
        const float s = sqrtf(h) + a.eps;
        const float q = g / s;
        const float x = fmaf(a.lr, q, a.X[tb][e]);
        a.H[tb][e] = h;
        a.X[tb][e] = x;
        a.A[tb][e] = 0;
        bad = bad || !gae::finite32(x) || !gae::finite32(h);
    }
    if (bad) or_bits(a.status, GAE_DEEPWALK_ERR_NONFINITE);
}

unsigned sweep_blocks(int64_t count)
{
    const int64_t b = cdiv(count, kThreads);
    return unsigned(b < 1 ? 1 : (b > kMaxGrid ? kMaxGrid : b));
}

} // namespace

extern "C" int gae_random_walks(const int64_t *indptr, const int32_t *indices, int64_t n, int64_t nnz, const int32_t *starts,
                                int64_t m, int64_t walks_per_start, int64_t length, uint64_t seed, int32_t *walks,
                                int64_t *status, void *stream)
{
    const char *fn = "gae_random_walks";
    GAE_REQUIRE(n >= 0 && nnz >= 0 && m >= 0, GAE_E_SIZE, "%s: negative n = %lld, nnz = %lld or m = %lld", fn, (long long)n,
                (long long)nnz, (long long)m);
    GAE_REQUIRE(n < (int64_t(1) << 31), GAE_E_SIZE, "%s: n = %lld beyond the int32 columns", fn, (long long)n);
    GAE_REQUIRE(length >= 1 && length <= kMaxWalkLength, GAE_E_RANGE, "%s: length = %lld outside 1..%d", fn, (long long)length,
                kMaxWalkLength);
    GAE_REQUIRE(walks_per_start >= 1 && walks_per_start < (int64_t(1) << 31), GAE_E_RANGE,
                "%s: walks_per_start = %lld outside 1..2^31 - 1", fn, (long long)walks_per_start);
    GAE_REQUIRE(m < (int64_t(1) << 31) && m * walks_per_start < (int64_t(1) << 31), GAE_E_SIZE,
                "%s: %lld starts times %lld walks is 2^31 or more", fn, (long long)m, (long long)walks_per_start);
    GAE_REQUIRE(starts || m <= n, GAE_E_SIZE, "%s: m = %lld beyond n = %lld without a start list", fn, (long long)m, (long long)n);
    GAE_REQUIRE(indptr && status, GAE_E_NULL, "%s: indptr / status is NULL", fn);
    GAE_REQUIRE(nnz == 0 || indices, GAE_E_NULL, "%s: indices is NULL", fn);
    GAE_REQUIRE(m == 0 || walks, GAE_E_NULL, "%s: walks is NULL", fn);
    if (m == 0) return GAE_OK;
    WalkArgs a;
    a.indptr = indptr; a.indices = indices; a.n = n; a.nnz = nnz;
    a.starts = starts; a.m = m; a.n_walks = m * walks_per_start;
    a.L = int(length); a.seed = seed; a.walks = walks; a.status = status;
    hipLaunchKernelGGL(random_walks_kernel, dim3(unsigned(cdiv(a.n_walks, kThreads))), dim3(kThreads), 0, gae::as_stream(stream),
                       a);
    GAE_CHECK_LAUNCH("random_walks_kernel");
    return GAE_OK;
}

extern "C" int gae_sgns_init(float *W, int64_t n, int64_t d, uint64_t seed, float bound, void *stream)
{
    const char *fn = "gae_sgns_init";
    GAE_REQUIRE(n >= 0 && n < (int64_t(1) << 31), GAE_E_SIZE, "%s: n = %lld outside 0..2^31 - 1", fn, (long long)n);
    GAE_REQUIRE(d >= 1 && d <= kMaxD, GAE_E_RANGE, "%s: d = %lld outside 1..%d", fn, (long long)d, kMaxD);
    GAE_REQUIRE(n == 0 || W, GAE_E_NULL, "%s: W is NULL", fn);
    if (n == 0) return GAE_OK;
    hipLaunchKernelGGL(sgns_init_kernel, dim3(sweep_blocks(n * d)), dim3(kThreads), 0, gae::as_stream(stream), W, n * d, seed,
                       bound);
    GAE_CHECK_LAUNCH("sgns_init_kernel");
    return GAE_OK;
}

extern "C" int gae_sgns_walk_order(int64_t n_walks, uint64_t seed, int64_t epoch, int32_t *order, void *stream)
{
    const char *fn = "gae_sgns_walk_order";
    GAE_REQUIRE(n_walks >= 0 && n_walks < (int64_t(1) << 31), GAE_E_SIZE, "%s: n_walks = %lld outside 0..2^31 - 1", fn,
                (long long)n_walks);
    GAE_REQUIRE(epoch >= 0 && epoch < (int64_t(1) << 31), GAE_E_RANGE, "%s: epoch = %lld outside 0..2^31 - 1", fn,
                (long long)epoch);
    GAE_REQUIRE(n_walks == 0 || order, GAE_E_NULL, "%s: order is NULL", fn);
    if (n_walks == 0) return GAE_OK;
    hipLaunchKernelGGL(sgns_order_kernel, dim3(unsigned(cdiv(n_walks, kThreads))), dim3(kThreads), 0, gae::as_stream(stream),
                       order, uint32_t(n_walks), gae::feistel::half_bits(uint64_t(n_walks)), seed, uint32_t(epoch));
    GAE_CHECK_LAUNCH("sgns_order_kernel");
    return GAE_OK;
}

namespace {

// the shape checks the two launches of a batch share
int check_tables(const char *fn, int64_t n, int64_t d)
{
    GAE_REQUIRE(d >= 1 && d <= kMaxD, GAE_E_RANGE, "%s: d = %lld outside 1..%d", fn, (long long)d, kMaxD);
    GAE_REQUIRE(n >= 1 && n < (int64_t(1) << 31), GAE_E_SIZE, "%s: n = %lld outside 1..2^31 - 1", fn, (long long)n);
    return GAE_OK;
}

} // namespace

extern "C" int gae_sgns_accumulate(const int32_t *walks, int64_t n_walks, int64_t length, const int32_t *order, int64_t first,
                                   int64_t count, const int64_t *cum, int64_t n, int64_t d, int64_t window, int64_t negatives,
                                   int64_t shared_negatives, uint64_t seed, int64_t epoch, const float *W, const float *C,
                                   int64_t *AW, int64_t *AC, int64_t *status, void *stream)
{
    const char *fn = "gae_sgns_accumulate";
    if (const int rc = check_tables(fn, n, d)) return rc;
    GAE_REQUIRE(length >= 2 && length <= kMaxL, GAE_E_RANGE, "%s: length = %lld outside 2..%d", fn, (long long)length, kMaxL);
    GAE_REQUIRE(window >= 1 && window < length, GAE_E_RANGE, "%s: window = %lld outside 1..length - 1 = %lld", fn,
                (long long)window, (long long)length - 1);
    GAE_REQUIRE(shared_negatives == 16 || shared_negatives == 32 || shared_negatives == 48 || shared_negatives == 64,
                GAE_E_RANGE, "%s: shared_negatives = %lld is not 16, 32, 48 or 64", fn, (long long)shared_negatives);
    GAE_REQUIRE(negatives >= 0 && negatives <= kMaxK, GAE_E_RANGE, "%s: negatives = %lld outside 0..%d", fn,
                (long long)negatives, kMaxK);
    GAE_REQUIRE(epoch >= 0 && epoch < (int64_t(1) << 31), GAE_E_RANGE, "%s: epoch = %lld outside 0..2^31 - 1", fn,
                (long long)epoch);
    GAE_REQUIRE(n_walks >= 1 && n_walks < (int64_t(1) << 31), GAE_E_SIZE, "%s: n_walks = %lld outside 1..2^31 - 1", fn,
                (long long)n_walks);
    GAE_REQUIRE(first >= 0 && count >= 0 && first + count <= n_walks, GAE_E_SIZE,
                "%s: positions [%lld, %lld + %lld) outside the %lld walks", fn, (long long)first, (long long)first,
                (long long)count, (long long)n_walks);
    GAE_REQUIRE(walks && order && cum && W && C && AW && AC && status, GAE_E_NULL,
                "%s: walks / order / cum / W / C / AW / AC / status is NULL", fn);
    if (count == 0) return GAE_OK;
    SgnsArgs a;
    a.walks = walks; a.order = order; a.n_walks = n_walks; a.first = first;
    a.L = int(length); a.LP = up16(a.L); a.d = int(d); a.dP = up16(a.d); a.M = int(shared_negatives);
    a.window = int(window); a.K = int(negatives);
    a.cum = cum; a.n = n; a.seed = seed; a.epoch = uint32_t(epoch);
    a.W = W; a.C = C; a.AW = AW; a.AC = AC; a.status = status;
    const Layout lay = make_layout(a.LP, a.dP, a.M);
    return gae::launch_lds<&sgns_accumulate_kernel>("sgns_accumulate_kernel", count, kThreads, size_t(lay.floats) * 4,
                                                    gae::as_stream(stream), a);
}

extern "C" int gae_sgns_update(float *W, float *C, float *HW, float *HC, int64_t *AW, int64_t *AC, int64_t n, int64_t d,
                               float lr, float eps, int64_t *status, void *stream)
{
    const char *fn = "gae_sgns_update";
    if (const int rc = check_tables(fn, n, d)) return rc;
    GAE_REQUIRE(lr > 0.f && lr <= FLT_MAX && eps > 0.f && eps <= FLT_MAX, GAE_E_RANGE, "%s: lr = %g or eps = %g is not positive and finite",
                fn, lr, eps);
    GAE_REQUIRE(W && C && HW && HC && AW && AC && status, GAE_E_NULL, "%s: W / C / HW / HC / AW / AC / status is NULL", fn);
    UpdateArgs a;
    a.X[0] = W; a.X[1] = C; a.H[0] = HW; a.H[1] = HC; a.A[0] = AW; a.A[1] = AC;
    a.count = n * d; a.lr = lr; a.eps = eps; a.status = status;
    hipLaunchKernelGGL(sgns_update_kernel, dim3(sweep_blocks(2 * a.count)), dim3(kThreads), 0, gae::as_stream(stream), a);
    GAE_CHECK_LAUNCH("sgns_update_kernel");
    return GAE_OK;
}
