// K32: spectral embedding of a graph (ops.spectral_embedding): Chebyshev-filtered block subspace iteration with a
// Rayleigh-Ritz step, fp64.
//
// The contract -- the operator, every chain, the Gram order, the small solve step by step, the filter's coefficients, the
// residuals, the sign rule, the status block -- is the K32 comment of include/gae_hip_experimental.h; tests/spectral_ref.py
// restates it in numpy.  This file is compiled without contraction: fma only where __builtin_fma is written.
//
// Launches (ordinary ones; no float atomics, integer atomics on counters and flags only):
//   spmm     a row goes to a group of g lanes, g the power of two >= b / 2 (1 .. 64): lane l of the group owns columns
//            2 l, 2 l + 1 (one 16-byte load per neighbour), 256 / g rows per block pass.  Four neighbours are in flight:
//            their ids, scales and operand pairs are loaded before the first fma, the fmas run in CSR order.  A hub row
//            is one group's serial chain (the sum is never split).
//   gram     one block of four waves per chunk of 256 rows; 16 rows at a time are staged in LDS (zero past b and n), the
//            2 . NT (NT + 1) / 2 upper-triangle tiles of V^T V and V^T AV are dealt round-robin to the waves (fold_lists.h's
//            tile deal and pitch; ridge.hip's operand layout: A lane l = v[4 s + (l >> 4)][16 ti + (l & 15)], D col = l & 15,
//            row = (l >> 4) + 4 reg).
//   reduce   fold_lists.h's reduce_entries: the chunk partials of an entry in the order of common.h's sum_partials.
//   solve    pre (Cholesky, the two triangular reductions, the packing) -- gae_pca_solve -- post (back substitution,
//            coefficients, status): one block each.  The b x b matrix sits in LDS (pitch b | 1), L in the workspace.
//   rotate   a block per chunk of 256 rows, 8 rows at a time: T (b x b) and the rows in LDS, one thread per (row, column)
//            item and both operands; the squared residual terms go back through LDS so that thread c adds column c's in
//            row order.  In place: a block owns its rows.
//   finish   chunk winners per column, one block folds them in chunk order, one elementwise pass writes.
//
// LDS: gram 2 . 16 . pitch . 8 (36 KB at b = 128); solve b (b | 1) 8 + 8 b (130 KB); rotate (b b + 2 . 8 b + b) 8 (145 KB).
#include "common.h"
#include "cholesky.h"
#include "fold_lists.h"

namespace {

using gae::cdiv;
using gae::finite64;
using gae::up256;
using gae::upper_at;
using gae::tri;
using gae::v4d;

constexpr int kMaxB = GAE_SPECTRAL_MAX_B, kMaxK = GAE_SPECTRAL_MAX_K, kMaxDegree = GAE_SPECTRAL_MAX_DEGREE;
constexpr int kChunk = GAE_SPECTRAL_CHUNK_ROWS;
constexpr int kThreads = 256, kWaves = kThreads / gae::kWave;
constexpr int kSolveThreads = 128;         // cholesky_crout: a thread per row
constexpr int kStage = 16;                 // gram: rows per LDS stage
constexpr int kRotRows = 8;                // rotate: rows per LDS pass
constexpr int kRotItems = kRotRows * kMaxB / kThreads;
constexpr int kMaxGrid = 8192;
static_assert(kChunk % kStage == 0 && kChunk % kRotRows == 0, "a chunk is a whole number of passes");

typedef double v2d __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------------------ the carve
// the regions the solve needs do not depend on n and come first
struct Regions {
    double *L, *stats, *mean, *W;
    gae_pca_status *pst;
    char *pca_ws;
    int64_t pca_ws_bytes;
    double *gram_part, *res_part, *best, *sign;
};

Regions carve(gae::Carver &cv, int64_t n, int64_t b)
{
    const int64_t chunks = cdiv(n, kChunk);
    Regions r;
    r.L = cv.take<double>(b * b);
    r.stats = cv.take<double>(tri(1 + b));
    r.mean = cv.take<double>(b);
    r.W = cv.take<double>(b * b);
    r.pst = cv.take<gae_pca_status>(1);
    r.pca_ws_bytes = gae_pca_workspace_bytes(b);
    r.pca_ws = cv.raw<char>(up256(r.pca_ws_bytes));
    r.gram_part = cv.take<double>(chunks * 2 * b * b);
    r.res_part = cv.take<double>(chunks * b);
    r.best = cv.take<double>(chunks * b);
    r.sign = cv.take<double>(b);
    return r;
}

int check_b(const char *fn, int64_t b)
{
    GAE_REQUIRE(b >= 2 && b <= kMaxB && (b & 1) == 0, GAE_E_RANGE, "%s: b = %lld must be even and in 2..128", fn, (long long)b);
    return GAE_OK;
}

int check_n(const char *fn, int64_t n)
{
    GAE_REQUIRE(n >= 1 && n < (int64_t(1) << 31), GAE_E_SIZE, "%s: n = %lld outside 1..2^31 - 1", fn, (long long)n);
    return GAE_OK;
}

int check_ws(const char *fn, const void *ws, int64_t have, int64_t n, int64_t b)
{
    GAE_REQUIRE(ws, GAE_E_NULL, "%s: workspace is NULL", fn);
    const int64_t need = gae_spectral_workspace_bytes(n, 0, b);
    GAE_REQUIRE(have >= need, GAE_E_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn, (long long)have, (long long)need);
    return GAE_OK;
}

// ------------------------------------------------------------------------------------------------------ scale, init
__global__ __launch_bounds__(kThreads) void spectral_scale_kernel(const int32_t *__restrict__ indptr, int n, double sigma,
                                                                  double *__restrict__ s)
{
    for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += int64_t(gridDim.x) * kThreads) {
        const double t = double(indptr[i + 1] - indptr[i]) + sigma;
        double v = 0.0;
        if (t > 0.0) {
            const double root = sqrt(t);
            v = 1.0 / root;
        }
        s[i] = v;
    }
}

__global__ __launch_bounds__(kThreads) void spectral_init_kernel(double *__restrict__ V, int64_t total, uint64_t key)
{
    const int64_t blocks = (total + 3) / 4;
    for (int64_t q = int64_t(blockIdx.x) * kThreads + threadIdx.x; q < blocks; q += int64_t(gridDim.x) * kThreads) {
        uint32_t w[4];
        gae::philox4x32_10(uint64_t(q), 0, key, w);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const double u1 = (double(w[2 * h] >> 8) + 0.5) * 0x1p-24;
            const double u2 = double(w[2 * h + 1] >> 8) * 0x1p-24;
            const double lg = log(u1);
            const double rad = sqrt(-2.0 * lg);
            const double ang = 6.283185307179586 * u2;
            const int64_t e = 4 * q + 2 * h;
            if (e < total) V[e] = rad * cos(ang);
            if (e + 1 < total) V[e + 1] = rad * sin(ang);
        }
    }
}

// ------------------------------------------------------------------------------------------------------ spmm
struct SpmmArgs {
    const int32_t *indptr, *indices;
    int n, nnz, b, g;                      // g lanes per row
    const double *s;
    double sigma;
    const double *Yin, *Yprev;
    double *Yout;
    const double *coef;
    gae_spectral_status *st;
};

__device__ __forceinline__ v2d fma2(double w, v2d y, v2d acc)
{
    return v2d{__builtin_fma(w, y[0], acc[0]), __builtin_fma(w, y[1], acc[1])};
}

__global__ __launch_bounds__(kThreads) void spectral_spmm_kernel(const SpmmArgs a)
{
    const int g = a.g, lg = threadIdx.x & (g - 1), rl = threadIdx.x / g, R = kThreads / g;
    const int nv = a.b >> 1, n = a.n;
    const double alpha = a.coef[0], beta = a.coef[1], gamma = a.coef[2];
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.st) gae::add_count(&a.st->n_spmm, 1);
    if (lg >= nv) return;
    bool bad = false;
    for (int64_t row = int64_t(blockIdx.x) * R + rl; row < n; row += int64_t(gridDim.x) * R) {
        int lo = a.indptr[row], hi = a.indptr[row + 1];
        if (lo < 0 || hi > a.nnz || lo > hi) { bad = true; lo = hi = 0; }
        const v2d *Yv = reinterpret_cast<const v2d *>(a.Yin) + lg;
        v2d acc = v2d{0.0, 0.0};
        int e = lo;
        for (; e + 4 <= hi; e += 4) {
            int j[4];
            double w[4];
            v2d y[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) j[u] = a.indices[e + u];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool ok = unsigned(j[u]) < unsigned(n);
                bad = bad || !ok;
                if (!ok) j[u] = int(row);
                w[u] = ok ? a.s[j[u]] : 0.0;
                y[u] = Yv[int64_t(j[u]) * nv];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = fma2(w[u], y[u], acc);
        }
        for (; e < hi; ++e) {
            int j = a.indices[e];
            const bool ok = unsigned(j) < unsigned(n);
            bad = bad || !ok;
            if (!ok) j = int(row);
            const double w = ok ? a.s[j] : 0.0;
            acc = fma2(w, Yv[int64_t(j) * nv], acc);
        }
        const double si = a.s[row];
        const v2d yi = Yv[row * nv];
        if (a.sigma != 0.0) {
            const double w = a.sigma * si;
            acc = fma2(w, yi, acc);
        }
        v2d o;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const double t = si * acc[u];
            const double at = alpha * t;
            o[u] = __builtin_fma(beta, yi[u], at);
        }
        if (a.Yprev) {
            const v2d yp = reinterpret_cast<const v2d *>(a.Yprev)[row * nv + lg];
            o = fma2(gamma, yp, o);
        }
        reinterpret_cast<v2d *>(a.Yout)[row * nv + lg] = o;
    }
    if (bad && a.st) gae::or_bits(&a.st->errors, GAE_SPECTRAL_ERR_INDEX);
}

// ------------------------------------------------------------------------------------------------------ gram
struct GramArgs {
    const double *V, *AV;
    int n, b;
    int64_t chunks;
    double *part;                          // [chunks][2][b][b]
    double *G, *H;
};

template <int NT>
__global__ __launch_bounds__(kThreads) void spectral_gram_kernel(const GramArgs a)
{
    constexpr int WP = 16 * NT, pitch = gae::tile_pitch(NT);
    constexpr int T = NT * (NT + 1) / 2, TPW = (2 * T + kWaves - 1) / kWaves;
    constexpr int PF = kStage * WP / kThreads;
    static_assert(PF * kThreads == kStage * WP, "a stage is a whole number of block passes");
    __shared__ __attribute__((aligned(16))) double buf[2 * kStage * pitch];
    double *Vs = buf, *As = buf + kStage * pitch;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = a.b;
    const int kr = lane >> 4, kc = lane & 15;

    int ti[TPW], tj[TPW], boff[TPW];
    bool mine[TPW], second[TPW];
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
        const int e = wave + kWaves * u;
        mine[u] = e < 2 * T;
        second[u] = e >= T;
        ti[u] = 0; tj[u] = 0;
        if (mine[u]) gae::upper_tile(second[u] ? e - T : e, NT, ti[u], tj[u]);
        boff[u] = (mine[u] && second[u]) ? kStage * pitch : 0;
    }

    for (int64_t chunk = blockIdx.x; chunk < a.chunks; chunk += gridDim.x) {
        const int64_t base = chunk * kChunk;
        const int nrows = a.n - base < kChunk ? int(a.n - base) : kChunk;
        const int nst = (nrows + kStage - 1) / kStage;
        v4d acc[TPW];
#pragma unroll
        for (int u = 0; u < TPW; ++u) acc[u] = v4d{0.0, 0.0, 0.0, 0.0};
        for (int it = 0; it < nst; ++it) {
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                const int e = tid + u * kThreads, r = e / WP, c = e % WP;
                const int64_t row = base + it * kStage + r;
                const bool on = row < a.n && c < b;
                Vs[r * pitch + c] = on ? a.V[row * b + c] : 0.0;
                As[r * pitch + c] = on ? a.AV[row * b + c] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < kStage / 4; ++s) {
                const double *rp = Vs + (4 * s + kr) * pitch + kc;
#pragma unroll
                for (int u = 0; u < TPW; ++u)
                    acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(rp[16 * ti[u]], rp[16 * tj[u] + boff[u]], acc[u], 0, 0, 0);
            }
            __syncthreads();
        }
        double *out = a.part + chunk * 2 * b * b;
#pragma unroll
        for (int u = 0; u < TPW; ++u) {
            if (!mine[u]) continue;
            double *o = out + (second[u] ? b * b : 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = 16 * ti[u] + kr + 4 * q, col = 16 * tj[u] + kc;
                if (row <= col && col < b) o[row * b + col] = acc[u][q];
            }
        }
    }
}

// entries e of [2][b][b] with i <= j: the chunk partials in the library's order (fold_lists.h's reduce_entries); the mirror
// is a copy
__global__ __launch_bounds__(kThreads) void spectral_gram_reduce_kernel(const GramArgs a)
{
    const int b = a.b;
    gae::reduce_entries<kThreads>(
        a.part, a.chunks, int64_t(2) * b * b, [&](int64_t e) { const int ij = int(e % (b * b)); return ij / b <= ij % b; },
        [&](int64_t e, double v) {
            const int which = int(e / (b * b)), ij = int(e % (b * b)), i = ij / b, j = ij % b;
            double *out = which ? a.H : a.G;
            out[i * b + j] = v;
            out[j * b + i] = v;
        });
}

// ------------------------------------------------------------------------------------------------------ solve
struct SolveArgs {
    const double *G, *H;
    int b, k, degree;
    double *L, *stats, *W, *T, *values, *coef;
    const gae_pca_status *pst;
    gae_spectral_status *st;
};

inline size_t solve_lds(int64_t b) { return size_t(b * (b | 1) + b) * 8; }

__global__ __launch_bounds__(kSolveThreads) void spectral_pre_kernel(const SolveArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int b = a.b, ld = b | 1, tid = threadIdx.x, W = 1 + b;
    double *M = lds, *dg = M + b * ld;
    for (int e = tid; e < b * b; e += kSolveThreads) M[(e / b) * ld + e % b] = a.G[e];
    __syncthreads();
    const int info = gae::cholesky_crout(M, dg, b, b, tid, [ld](int i) { return i * ld; });
    if (tid == 0) a.st->info = info;
    if (info != 0) {                                                   // the same value in every thread
        if (tid == 0) a.stats[0] = 0.0;                                // K31 then reports NaN (its info -1)
        return;
    }
    for (int e = tid; e < b * b; e += kSolveThreads) {
        const int i = e / b, j = e % b;
        a.L[e] = j < i ? M[i * ld + j] : (j == i ? dg[i] : 0.0);
    }
    __syncthreads();
    for (int e = tid; e < b * b; e += kSolveThreads) M[(e / b) * ld + e % b] = a.H[e];
    __syncthreads();
    const double *L = a.L;
    if (tid < b) {                                                     // X = L^-1 H, column tid
        const int c = tid;
        for (int i = 0; i < b; ++i) {
            double x = M[i * ld + c];
            for (int k = 0; k < i; ++k) {
                const double p = L[i * b + k] * M[k * ld + c];
                x = x - p;
            }
            M[i * ld + c] = x / dg[i];
        }
    }
    __syncthreads();
    if (tid < b) {                                                     // H' = X L^-T, row tid
        const int r = tid;
        for (int j = 0; j < b; ++j) {
            double y = M[r * ld + j];
            for (int k = 0; k < j; ++k) {
                const double p = L[j * b + k] * M[r * ld + k];
                y = y - p;
            }
            M[r * ld + j] = y / dg[j];
        }
    }
    __syncthreads();
    for (int e = tid; e < W; e += kSolveThreads) a.stats[e] = e == 0 ? 2.0 : 0.0;
    for (int e = tid; e < b * b; e += kSolveThreads) {
        const int i = e / b, j = e % b;
        if (i <= j) a.stats[upper_at(1 + i, 1 + j, W)] = M[i * ld + j];
    }
}

__global__ __launch_bounds__(kSolveThreads) void spectral_post_kernel(const SolveArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ int s_info;
    const int b = a.b, ld = b | 1, tid = threadIdx.x;
    double *Tm = lds;
    const double nan = __builtin_nan("");
    if (tid == 0) {
        int info = int(a.st->info);
        if (info == 0 && a.pst->info != 0) info = -1;
        if (info == 0)
            for (int c = 0; c < b; ++c)
                if (!finite64(a.values[c])) info = -2;
        s_info = info;
    }
    __syncthreads();
    const int info = s_info;
    if (info != 0) {
        for (int e = tid; e < b * b; e += kSolveThreads) a.T[e] = nan;
        for (int e = tid; e < b; e += kSolveThreads) a.values[e] = nan;
        if (tid == 0) { a.st->info = info; a.st->theta_1 = nan; a.st->theta_k = nan; }
        return;
    }
    const double *L = a.L;
    if (tid < b) {                                                     // T = L^-T W^T, column tid
        const int c = tid;
        for (int i = b - 1; i >= 0; --i) {
            double x = a.W[c * b + i];
            for (int k = i + 1; k < b; ++k) {
                const double p = L[k * b + i] * Tm[k * ld + c];
                x = x - p;
            }
            Tm[i * ld + c] = x / L[i * b + i];
        }
    }
    __syncthreads();
    for (int e = tid; e < b * b; e += kSolveThreads) a.T[e] = Tm[(e / b) * ld + e % b];
    if (tid == 0) {
        const double t1 = a.values[0], tk = a.values[a.k - 1], tb = a.values[b - 1];
        const double floor_ = tk - 0.02;
        double lim = tb < floor_ ? tb : floor_;
        if (lim < -0.5) lim = -0.5;
        const double e = (lim + 1.0) * 0.5, c = (lim - 1.0) * 0.5;
        const double s1 = e / (t1 - c);
        double *co = a.coef;
        co[0] = 1.0; co[1] = 0.0; co[2] = 0.0;
        double alpha = s1 / e;
        co[3] = alpha; co[4] = -(c * alpha); co[5] = 0.0;
        double s = s1;
        for (int d = 2; d <= a.degree; ++d) {
            const double s2 = 1.0 / (2.0 / s1 - s);
            alpha = (2.0 * s2) / e;
            co[3 * d] = alpha; co[3 * d + 1] = -(c * alpha); co[3 * d + 2] = -(s * s2);
            s = s2;
        }
        a.st->info = 0;
        a.st->theta_1 = t1;
        a.st->theta_k = tk;
    }
}

// ------------------------------------------------------------------------------------------------------ rotate
struct RotArgs {
    double *V, *AV;
    int n, b, k;
    int64_t chunks;
    const double *T, *values;
    double tol;
    double *part;                          // [chunks][b]
    double *res;
    gae_spectral_status *st;
};

inline size_t rotate_lds(int64_t b) { return size_t(b * b + 2 * kRotRows * b + b) * 8; }

__global__ __launch_bounds__(kThreads) void spectral_rotate_kernel(const RotArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int b = a.b, tid = threadIdx.x, items = kRotRows * b;
    double *Ts = lds, *Vs = Ts + b * b, *As = Vs + items, *th = As + items;
    for (int e = tid; e < b * b; e += kThreads) Ts[e] = a.T[e];
    for (int e = tid; e < b; e += kThreads) th[e] = a.values[e];
    __syncthreads();
    for (int64_t chunk = blockIdx.x; chunk < a.chunks; chunk += gridDim.x) {
        const int64_t base = chunk * kChunk;
        double racc = 0.0;
        for (int p = 0; p < kChunk / kRotRows; ++p) {
            const int64_t r0 = base + p * kRotRows;
            if (r0 >= a.n) break;                                      // the same in every thread
            for (int e = tid; e < items; e += kThreads) {
                const int64_t row = r0 + e / b;
                const bool on = row < a.n;
                Vs[e] = on ? a.V[r0 * b + e] : 0.0;
                As[e] = on ? a.AV[r0 * b + e] : 0.0;
            }
            __syncthreads();
            double ov[kRotItems], oa[kRotItems];
#pragma unroll
            for (int u = 0; u < kRotItems; ++u) {
                const int e = tid + u * kThreads;
                ov[u] = 0.0; oa[u] = 0.0;
                if (e < items) {
                    const int r = e / b, c = e % b;
                    const double *vr = Vs + r * b, *ar = As + r * b, *tc = Ts + c;
                    double x = 0.0, y = 0.0;
                    for (int j = 0; j < b; ++j) {
                        const double t = tc[j * b];
                        x = __builtin_fma(vr[j], t, x);
                        y = __builtin_fma(ar[j], t, y);
                    }
                    ov[u] = x; oa[u] = y;
                }
            }
            __syncthreads();                                           // every read of the staged rows is done
#pragma unroll
            for (int u = 0; u < kRotItems; ++u) {
                const int e = tid + u * kThreads;
                if (e < items) {
                    const int64_t row = r0 + e / b;
                    const int c = e % b;
                    double dd = 0.0;
                    if (row < a.n) {
                        a.V[r0 * b + e] = ov[u];
                        a.AV[r0 * b + e] = oa[u];
                        const double pr = th[c] * ov[u];
                        const double d = oa[u] - pr;
                        dd = d * d;
                    }
                    Vs[e] = dd;
                }
            }
            __syncthreads();
            if (tid < b)
                for (int r = 0; r < kRotRows; ++r) racc = racc + Vs[r * b + tid];
            __syncthreads();
        }
        if (tid < b) a.part[chunk * b + tid] = racc;
    }
}

__global__ __launch_bounds__(kThreads) void spectral_residual_kernel(const RotArgs a)
{
    __shared__ double res[kMaxB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = a.b;
    const int64_t P = a.chunks;
    const int L = gae::partial_lanes(P);
    for (int c = wave; c < b; c += kWaves) {                           // all 64 lanes of the wave call
        double s = 0.0;
        if (L == 64) s = gae::sum_partials(a.part + c, P, b, lane, 64);
        else if (lane == 0) s = gae::sum_partials(a.part + c, P, b, 0, 1);
        if (lane == 0) {
            const double r = sqrt(s);
            res[c] = r;
            a.res[c] = r;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int conv = 0, bad = 0;
        bool run = true;
        double worst = 0.0;
        for (int c = 0; c < a.k; ++c) {
            const double r = res[c];
            if (!finite64(r)) ++bad;
            if (run && r <= a.tol) ++conv; else run = false;
            if (r > worst) worst = r;
        }
        a.st->n_converged = conv;
        a.st->nonfinite = bad;
        a.st->res_max = bad ? __builtin_nan("") : worst;
    }
}

// ------------------------------------------------------------------------------------------------------ finish
struct FinArgs {
    const double *V;
    int n, b, first, k, scaling;
    int64_t chunks;
    const double *values, *s;
    double *best, *sign;                   // [chunks][k], [k]
    double *vectors;
    float *embedding;
};

__global__ __launch_bounds__(kThreads) void spectral_best_kernel(const FinArgs a)
{
    const int c = threadIdx.x;
    if (c >= a.k) return;
    for (int64_t chunk = blockIdx.x; chunk < a.chunks; chunk += gridDim.x) {
        const int64_t base = chunk * kChunk;
        const int nrows = a.n - base < kChunk ? int(a.n - base) : kChunk;
        double mag = -1.0, at = 0.0;
        for (int r = 0; r < nrows; ++r) {
            const double v = a.V[(base + r) * a.b + a.first + c];
            if (fabs(v) > mag) { mag = fabs(v); at = v; }
        }
        a.best[chunk * a.k + c] = at;
    }
}

__global__ __launch_bounds__(kThreads) void spectral_sign_kernel(const FinArgs a)
{
    const int c = threadIdx.x;
    if (c >= a.k) return;
    double mag = -1.0, at = 0.0;
    for (int64_t q = 0; q < a.chunks; ++q) {
        const double v = a.best[q * a.k + c];
        if (fabs(v) > mag) { mag = fabs(v); at = v; }
    }
    a.sign[c] = at < 0.0 ? -1.0 : 1.0;
}

__global__ __launch_bounds__(kThreads) void spectral_write_kernel(const FinArgs a)
{
    const int64_t total = int64_t(a.n) * a.k;
    for (int64_t e = int64_t(blockIdx.x) * kThreads + threadIdx.x; e < total; e += int64_t(gridDim.x) * kThreads) {
        const int64_t i = e / a.k;
        const int c = int(e % a.k);
        const double v = a.sign[c] * a.V[i * a.b + a.first + c];
        a.vectors[e] = v;
        double z = v;
        if (a.scaling == GAE_SPECTRAL_SCALE_DEGREE) {
            z = v * a.s[i];
        } else if (a.scaling == GAE_SPECTRAL_SCALE_VALUE) {
            const double t = a.values[a.first + c];
            const double root = sqrt(t > 0.0 ? t : 0.0);
            z = v * root;
        }
        a.embedding[e] = float(z);
    }
}

int64_t grid_for(int64_t items) { return items < kMaxGrid ? (items < 1 ? 1 : items) : kMaxGrid; }

template <int NT>
int launch_gram(const GramArgs &a, int64_t blocks, hipStream_t st)
{
    hipLaunchKernelGGL(spectral_gram_kernel<NT>, dim3(unsigned(blocks)), dim3(kThreads), 0, st, a);
    GAE_CHECK_LAUNCH("spectral_gram_kernel");
    return GAE_OK;
}

} // namespace

extern "C" int64_t gae_spectral_workspace_bytes(int64_t n, int64_t nnz, int64_t b)
{
    const char *fn = "gae_spectral_workspace_bytes";
    if (const int rc = check_b(fn, b)) return rc;
    if (const int rc = check_n(fn, n)) return rc;
    GAE_REQUIRE(nnz >= 0 && nnz < (int64_t(1) << 31), GAE_E_SIZE, "%s: nnz = %lld outside 0..2^31 - 1", fn, (long long)nnz);
    gae::Carver cv(nullptr);
    carve(cv, n, b);
    return cv.bytes();
}

extern "C" int gae_spectral_scale(const int32_t *indptr, int64_t n, double sigma, double *s, void *stream)
{
    const char *fn = "gae_spectral_scale";
    GAE_REQUIRE(sigma >= 0.0 && sigma <= DBL_MAX, GAE_E_RANGE, "%s: sigma = %g must be finite and >= 0", fn, sigma);
    if (const int rc = check_n(fn, n)) return rc;
    GAE_REQUIRE(indptr && s, GAE_E_NULL, "%s: indptr / s is NULL", fn);
    hipLaunchKernelGGL(spectral_scale_kernel, dim3(unsigned(grid_for(cdiv(n, kThreads)))), dim3(kThreads), 0,
                       gae::as_stream(stream), indptr, int(n), sigma, s);
    GAE_CHECK_LAUNCH("spectral_scale_kernel");
    return GAE_OK;
}

extern "C" int gae_spectral_init(double *V, int64_t n, int64_t b, uint64_t seed, void *stream)
{
    const char *fn = "gae_spectral_init";
    if (const int rc = check_b(fn, b)) return rc;
    if (const int rc = check_n(fn, n)) return rc;
    GAE_REQUIRE(V, GAE_E_NULL, "%s: V is NULL", fn);
    const int64_t total = n * b;
    hipLaunchKernelGGL(spectral_init_kernel, dim3(unsigned(grid_for(cdiv(cdiv(total, 4), kThreads)))), dim3(kThreads), 0,
                       gae::as_stream(stream), V, total, seed ^ uint64_t(GAE_SPECTRAL_KEY_XOR));
    GAE_CHECK_LAUNCH("spectral_init_kernel");
    return GAE_OK;
}

extern "C" int gae_spectral_spmm(const int32_t *indptr, const int32_t *indices, int64_t n, int64_t nnz, const double *s,
                                 double sigma, const double *Yin, const double *Yprev, double *Yout, int64_t b,
                                 const double *coef_dev, gae_spectral_status *status, void *stream)
{
    const char *fn = "gae_spectral_spmm";
    if (const int rc = check_b(fn, b)) return rc;
    GAE_REQUIRE(sigma >= 0.0 && sigma <= DBL_MAX, GAE_E_RANGE, "%s: sigma = %g must be finite and >= 0", fn, sigma);
    if (const int rc = check_n(fn, n)) return rc;
    GAE_REQUIRE(nnz >= 0 && nnz < (int64_t(1) << 31), GAE_E_SIZE, "%s: nnz = %lld outside 0..2^31 - 1", fn, (long long)nnz);
    GAE_REQUIRE(indptr && (indices || nnz == 0) && s, GAE_E_NULL, "%s: indptr / indices / s is NULL", fn);
    GAE_REQUIRE(Yin && Yout && coef_dev, GAE_E_NULL, "%s: Yin / Yout / coef_dev is NULL", fn);
    GAE_REQUIRE(Yin != Yout, GAE_E_SIZE, "%s: Yout aliases Yin", fn);
    GAE_REQUIRE(gae::aligned16(Yin) && gae::aligned16(Yout) && gae::aligned16(Yprev), GAE_E_SIZE,
                "%s: the operands must be 16-byte aligned", fn);
    int g = 1;
    while (g < b / 2) g *= 2;
    const SpmmArgs a{indptr, indices, int(n), int(nnz), int(b), g, s, sigma, Yin, Yprev, Yout, coef_dev, status};
    hipLaunchKernelGGL(spectral_spmm_kernel, dim3(unsigned(grid_for(cdiv(n, kThreads / g)))), dim3(kThreads), 0,
                       gae::as_stream(stream), a);
    GAE_CHECK_LAUNCH("spectral_spmm_kernel");
    return GAE_OK;
}

extern "C" int gae_spectral_gram(const double *V, const double *AV, int64_t n, int64_t b, double *G, double *H,
                                 int64_t max_blocks, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "gae_spectral_gram";
    if (const int rc = check_b(fn, b)) return rc;
    if (const int rc = check_n(fn, n)) return rc;
    GAE_REQUIRE(max_blocks >= 0, GAE_E_SIZE, "%s: negative max_blocks = %lld", fn, (long long)max_blocks);
    GAE_REQUIRE(V && AV && G && H, GAE_E_NULL, "%s: V / AV / G / H is NULL", fn);
    if (const int rc = check_ws(fn, workspace, workspace_bytes, n, b)) return rc;
    gae::Carver cv(workspace);
    const Regions r = carve(cv, n, b);
    const int64_t chunks = cdiv(n, kChunk);
    const GramArgs a{V, AV, int(n), int(b), chunks, r.gram_part, G, H};
    int64_t blocks = grid_for(chunks);
    if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
    hipStream_t st = gae::as_stream(stream);
    int rc = GAE_OK;
    switch (int(cdiv(b, 16))) {
    case 1: rc = launch_gram<1>(a, blocks, st); break;
    case 2: rc = launch_gram<2>(a, blocks, st); break;
    case 3: rc = launch_gram<3>(a, blocks, st); break;
    case 4: rc = launch_gram<4>(a, blocks, st); break;
    case 5: rc = launch_gram<5>(a, blocks, st); break;
    case 6: rc = launch_gram<6>(a, blocks, st); break;
    case 7: rc = launch_gram<7>(a, blocks, st); break;
    default: rc = launch_gram<8>(a, blocks, st); break;
    }
    if (rc) return rc;
    const int64_t E = 2 * b * b;
    const int64_t rblocks = chunks <= 32 ? cdiv(E, kThreads) : cdiv(E, kWaves * gae::kWaveEntries);
    hipLaunchKernelGGL(spectral_gram_reduce_kernel, dim3(unsigned(rblocks)), dim3(kThreads), 0, st, a);
    GAE_CHECK_LAUNCH("spectral_gram_reduce_kernel");
    return GAE_OK;
}

extern "C" int gae_spectral_solve(const double *G, const double *H, int64_t b, int64_t k, int64_t degree, double *T,
                                  double *values, double *coef, gae_spectral_status *status, void *workspace,
                                  int64_t workspace_bytes, void *stream)
{
    const char *fn = "gae_spectral_solve";
    if (const int rc = check_b(fn, b)) return rc;
    GAE_REQUIRE(k >= 1 && k <= kMaxK && k <= b, GAE_E_RANGE, "%s: k = %lld outside 1..min(b, 64)", fn, (long long)k);
    GAE_REQUIRE(degree >= 1 && degree <= kMaxDegree, GAE_E_RANGE, "%s: degree = %lld outside 1..12", fn, (long long)degree);
    GAE_REQUIRE(G && H && T && values && coef && status, GAE_E_NULL, "%s: G / H / T / values / coef / status is NULL", fn);
    if (const int rc = check_ws(fn, workspace, workspace_bytes, 1, b)) return rc;
    gae::Carver cv(workspace);
    const Regions r = carve(cv, 1, b);
    const SolveArgs a{G, H, int(b), int(k), int(degree), r.L, r.stats, r.W, T, values, coef, r.pst, status};
    hipStream_t st = gae::as_stream(stream);
    if (const int rc = gae::launch_lds<&spectral_pre_kernel>("spectral_pre_kernel", 1, kSolveThreads, solve_lds(b), st, a))
        return rc;
    if (const int rc = gae_pca_solve(r.stats, b, 0, nullptr, 2, b, 0, r.mean, values, r.W, r.pst, r.pca_ws, r.pca_ws_bytes,
                                     stream))
        return rc;
    return gae::launch_lds<&spectral_post_kernel>("spectral_post_kernel", 1, kSolveThreads, solve_lds(b), st, a);
}

extern "C" int gae_spectral_rotate(double *V, double *AV, int64_t n, int64_t b, int64_t k, const double *T,
                                   const double *values, double tol, double *residuals, gae_spectral_status *status,
                                   void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "gae_spectral_rotate";
    if (const int rc = check_b(fn, b)) return rc;
    GAE_REQUIRE(k >= 1 && k <= kMaxK && k <= b, GAE_E_RANGE, "%s: k = %lld outside 1..min(b, 64)", fn, (long long)k);
    GAE_REQUIRE(tol >= 0.0 && tol <= DBL_MAX, GAE_E_RANGE, "%s: tol = %g must be finite and >= 0", fn, tol);
    if (const int rc = check_n(fn, n)) return rc;
    GAE_REQUIRE(V && AV && T && values && residuals && status, GAE_E_NULL,
                "%s: V / AV / T / values / residuals / status is NULL", fn);
    GAE_REQUIRE(V != AV, GAE_E_SIZE, "%s: AV aliases V", fn);
    if (const int rc = check_ws(fn, workspace, workspace_bytes, n, b)) return rc;
    gae::Carver cv(workspace);
    const Regions r = carve(cv, n, b);
    const int64_t chunks = cdiv(n, kChunk);
    const RotArgs a{V, AV, int(n), int(b), int(k), chunks, T, values, tol, r.res_part, residuals, status};
    hipStream_t st = gae::as_stream(stream);
    if (const int rc = gae::launch_lds<&spectral_rotate_kernel>("spectral_rotate_kernel", grid_for(chunks), kThreads,
                                                                rotate_lds(b), st, a))
        return rc;
    hipLaunchKernelGGL(spectral_residual_kernel, dim3(1), dim3(kThreads), 0, st, a);
    GAE_CHECK_LAUNCH("spectral_residual_kernel");
    return GAE_OK;
}

extern "C" int gae_spectral_finish(const double *V, int64_t n, int64_t b, int64_t first, int64_t k, const double *values,
                                   const double *s, int scaling, double *vectors, float *embedding, void *workspace,
                                   int64_t workspace_bytes, void *stream)
{
    const char *fn = "gae_spectral_finish";
    if (const int rc = check_b(fn, b)) return rc;
    GAE_REQUIRE(k >= 1 && k <= kMaxK && k <= b, GAE_E_RANGE, "%s: k = %lld outside 1..min(b, 64)", fn, (long long)k);
    GAE_REQUIRE(scaling >= GAE_SPECTRAL_SCALE_NONE && scaling <= GAE_SPECTRAL_SCALE_VALUE, GAE_E_RANGE,
                "%s: unknown scaling %d", fn, scaling);
    if (const int rc = check_n(fn, n)) return rc;
    GAE_REQUIRE(first >= 0 && first + k <= b, GAE_E_SIZE, "%s: columns %lld .. %lld outside the block of %lld", fn,
                (long long)first, (long long)(first + k - 1), (long long)b);
    GAE_REQUIRE(V && values && s && vectors && embedding, GAE_E_NULL, "%s: V / values / s / vectors / embedding is NULL", fn);
    if (const int rc = check_ws(fn, workspace, workspace_bytes, n, b)) return rc;
    gae::Carver cv(workspace);
    const Regions r = carve(cv, n, b);
    const int64_t chunks = cdiv(n, kChunk);
    const FinArgs a{V, int(n), int(b), int(first), int(k), scaling, chunks, values, s, r.best, r.sign, vectors, embedding};
    hipStream_t st = gae::as_stream(stream);
    hipLaunchKernelGGL(spectral_best_kernel, dim3(unsigned(grid_for(chunks))), dim3(kThreads), 0, st, a);
    GAE_CHECK_LAUNCH("spectral_best_kernel");
    hipLaunchKernelGGL(spectral_sign_kernel, dim3(1), dim3(kThreads), 0, st, a);
    GAE_CHECK_LAUNCH("spectral_sign_kernel");
    hipLaunchKernelGGL(spectral_write_kernel, dim3(unsigned(grid_for(cdiv(n * k, kThreads)))), dim3(kThreads), 0, st, a);
    GAE_CHECK_LAUNCH("spectral_write_kernel");
    return GAE_OK;
}
