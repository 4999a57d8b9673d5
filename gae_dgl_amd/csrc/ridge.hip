// K25: ridge regression on frozen features with a k-fold CV lambda path (ops.ridge, GAE.ridge_graphs).
//
// X fp32 [n, d] (ldx), Y fp32 [n, t] (ldy); 1 <= d <= 128, 1 <= t <= 8, 1 <= F <= 32 folds, 1 <= L <= 64 lambdas.  The
// contract -- the moments, their packing, the order of every sum, the status block, info -- is the comment of
// gae_ridge_stats / gae_ridge_solve in include/gae_hip_experimental.h.
//
// Launches (ordinary ones, no float atomics):
//   stats   one block of four waves per chunk of GAE_RIDGE_CHUNK_ROWS listed rows of ONE fold (fold_lists.h: the fold list,
//           the chunk order, the row-id fetch, the tile deal and the pitch).  The block stages 32 rows
//           at a time in LDS as v = [1, x - p_x, y - p_y] in fp64 (widened first, then subtracted), zero past W and past
//           the chunk: two LDS buffers and two register sets, the global loads of stage s + 2 issued before the products
//           of stage s, one barrier per stage.  M = sum_i v_i v_i^T runs on v_mfma_f64_16x16x4_f64: W is padded to NT tiles of 16, the
//           NT (NT + 1) / 2 upper-triangle tiles are dealt round-robin to the waves (at NT = 9: 45 tiles, 12 per wave at
//           most, 4 fp64 per lane each), one wave walks all rows of the chunk for its tiles in ascending order.  A: lane l
//           holds v[row 4 s + (l >> 4)][16 ti + (l & 15)], B the same with tj; D: col = l & 15, row = (l >> 4) + 4 reg.
//           The packed upper triangle of the chunk goes to the workspace.  Rows that hold a non-finite value are counted
//           through a bit mask per stage in LDS (integer atomics), row ids outside [0, n) are flagged and skipped.
//   reduce  fold_lists.h's reduce_entries per fold: the fold's chunk partials in the order of common.h's sum_partials, in
//           fp64.
//   solve   one block per (model, lambda): the training moments (folds other than the model's, ascending), centring,
//           + lambda I, a Cholesky-Crout factorisation of the packed lower triangle in LDS whose row loop also carries
//           the t right-hand sides (forward substitution), back substitution, the map back through the pivot, and the
//           held-out SSE as a quadratic form of the fold's own moments.
//
// LDS: stats 2 . 32 . pitch . 8 + 1 KB of row ids + the pivot (76 KB at W = 137); solve (d (d + 1) / 2 + 2 t d + d +
// 4 (d + t) + t + 8) . 8 bytes (87 KB at d = 128, t = 8).
#include "common.h"
#include "cholesky.h"
#include "fold_lists.h"

namespace {

using gae::cdiv;
using gae::up256;

constexpr int kMaxD = 128, kMaxT = 8, kMaxF = 32, kMaxL = 64;
constexpr int kChunk = GAE_RIDGE_CHUNK_ROWS;
constexpr int kStage = 32;                 // rows per LDS stage: eight products of four rows
constexpr int kThreads = 256, kWaves = kThreads / gae::kWave;
static_assert(kChunk % kStage == 0, "a chunk is a whole number of stages");

using gae::tri;
using gae::upper_at;
using gae::v4d;

// ------------------------------------------------------------------------------------------------------ stats
struct StatsArgs {
    const float *X, *Y;
    int64_t ldx, ldy;
    int n, d, t, W;
    const float *pivot;                    // [d + t] or NULL
    gae::FoldList list;                    // the listed rows (fold_lists.h)
    double *part;                          // [chunks][tri(W)]
    double *stats;                         // [F][tri(W)]
    gae_ridge_status *status;
};

template <int NT>
__global__ __launch_bounds__(kThreads) void ridge_stats_kernel(const StatsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int WP = 16 * NT, pitch = gae::tile_pitch(NT);
    constexpr int T = NT * (NT + 1) / 2, TPW = (T + kWaves - 1) / kWaves;
    constexpr int PF = kStage * WP / kThreads;                         // staged values per thread and stage
    constexpr int kGroup = NT >= 9 ? 1 : 8;                            // ... whose LDS reads are issued together (NT = 9: registers)
    static_assert(PF * kThreads == kStage * WP, "a stage is a whole number of block passes");
    double *buf = lds;                                                 // [2][kStage][pitch]
    double *pv = buf + 2 * kStage * pitch;                             // [WP]: 0, p_x, p_y, 0 ...
    int *rid = reinterpret_cast<int *>(pv + WP);                       // [kChunk]: row ids, -1 = no row
    unsigned *mask = reinterpret_cast<unsigned *>(rid + kChunk);       // [2]: rows of a stage that hold a non-finite value
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    if (!gae::folds_valid(a.list)) {
        if (blockIdx.x == 0 && tid == 0) gae::or_bits(&a.status->errors, GAE_RIDGE_ERR_FOLD_PTR);
        return;
    }
    const gae::Chunk ch = gae::chunk_of(a.list, blockIdx.x, kChunk);   // the block's chunk
    if (ch.fold < 0) return;                                           // a spare block of the grid's upper bound
    const int lo = ch.lo, nrows = ch.hi - ch.lo, nst = (nrows + kStage - 1) / kStage;

    bool bad_id = false;
    for (int i = tid; i < kChunk; i += kThreads)
        rid[i] = i < nrows ? gae::row_id(a.list, lo + i, a.n, bad_id) : -1;
    if (bad_id) gae::or_bits(&a.status->errors, GAE_RIDGE_ERR_ROW_ID);
    for (int c = tid; c < WP; c += kThreads)
        pv[c] = (a.pivot && c >= 1 && c <= a.d + a.t) ? double(a.pivot[c - 1]) : 0.0;
    if (tid < 2) mask[tid] = 0u;
    __syncthreads();

    // ---- the wave's tiles: e = wave, wave + 4, ... of the upper-triangle tiles in row order
    // (a slot past the last tile repeats tile (0, 0) and is not stored: the product loop stays free of branches, so the
    // LDS reads of the next products are issued under the current ones)
    int ti[TPW], tj[TPW];
    bool mine[TPW];
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
        const int e = wave + kWaves * u;
        ti[u] = 0; tj[u] = 0;
        mine[u] = e < T;
        if (e < T) gae::upper_tile(e, NT, ti[u], tj[u]);
    }
    v4d acc[TPW];
#pragma unroll
    for (int u = 0; u < TPW; ++u) acc[u] = v4d{0.0, 0.0, 0.0, 0.0};

    // ---- staging: element e = tid + u 256 of a stage is row e / WP, column e % WP.  Two register sets: the loads of
    // stage it + 2 are issued before the products of stage it and written to LDS after the products of stage it + 1
    float pfa[PF], pfb[PF];
    unsigned livea = 0, liveb = 0;
    auto fetch = [&](int it, float (&pf)[PF], unsigned &live) {
        live = 0;
        if (it >= nst) return;
        // in groups of kGroup values: the row ids of a group are read together, then its loads are issued
#pragma unroll
        for (int u0 = 0; u0 < PF; u0 += kGroup) {
            int id[kGroup];
#pragma unroll
            for (int u = u0; u < u0 + kGroup && u < PF; ++u) id[u - u0] = rid[it * kStage + (tid + u * kThreads) / WP];
#pragma unroll
            for (int u = u0; u < u0 + kGroup && u < PF; ++u) {
                const int c = (tid + u * kThreads) % WP, i = id[u - u0];
                const bool on = i >= 0 && c <= a.d + a.t;
                float v = c == 0 ? 1.f : 0.f;
                if constexpr (kGroup > 1) {                            // one address for every lane, one load under `on`
                    const float *src = c <= a.d ? a.X + (int64_t(i) * a.ldx + (c - 1)) : a.Y + (int64_t(i) * a.ldy + (c - 1 - a.d));
                    if (on && c > 0) v = *src;
                } else if (on && c > 0) {                              // (the widest form has no registers for both addresses)
                    v = c <= a.d ? a.X[int64_t(i) * a.ldx + (c - 1)] : a.Y[int64_t(i) * a.ldy + (c - 1 - a.d)];
                }
                pf[u] = on ? v : 0.f;
                live |= (on ? 1u : 0u) << u;
            }
        }
    };
    auto stash = [&](int it, const float (&pf)[PF], unsigned live) {
        if (it >= nst) return;
        double *dst = buf + (it & 1) * kStage * pitch;
#pragma unroll
        for (int u0 = 0; u0 < PF; u0 += kGroup) {                      // a group's pivots are read before its first write: one wait
            double p[kGroup];
#pragma unroll
            for (int u = u0; u < u0 + kGroup && u < PF; ++u) p[u - u0] = pv[(tid + u * kThreads) % WP];
#pragma unroll
            for (int u = u0; u < u0 + kGroup && u < PF; ++u) {
                const int e = tid + u * kThreads, r = e / WP, c = e % WP;
                const bool on = (live >> u) & 1u;
                if (on && !gae::finite32(pf[u])) atomicOr(&mask[it & 1], 1u << r);
                dst[r * pitch + c] = on ? double(pf[u]) - p[u - u0] : 0.0;
            }
        }
    };
    unsigned bad_rows = 0;
    const int kr = lane >> 4, kc = lane & 15;
    auto products = [&](int it) {
        const double *bp = buf + (it & 1) * kStage * pitch;
#pragma unroll
        for (int s = 0; s < kStage / 4; ++s) {
            const double *rp = bp + (4 * s + kr) * pitch + kc;
#pragma unroll
            for (int u = 0; u < TPW; ++u)
                acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(rp[16 * ti[u]], rp[16 * tj[u]], acc[u], 0, 0, 0);
            if constexpr (TPW > 9) __builtin_amdgcn_sched_barrier(0);  // 12 tiles: operands hoisted further would spill
        }
        if (tid == 0) { bad_rows += __popc(mask[it & 1]); mask[it & 1] = 0u; }
    };
    fetch(0, pfa, livea);
    fetch(1, pfb, liveb);
    stash(0, pfa, livea);
    __syncthreads();
    for (int it = 0; it < nst; it += 2) {                              // stage it is in LDS, stage it + 1 in set b
        fetch(it + 2, pfa, livea);
        products(it);
        stash(it + 1, pfb, liveb);                                     // the buffer stage it - 1 read; every wave is past that barrier
        __syncthreads();
        if (it + 1 >= nst) break;
        fetch(it + 3, pfb, liveb);
        products(it + 1);
        stash(it + 2, pfa, livea);
        __syncthreads();
    }

    // ---- the chunk's packed upper triangle
    double *out = a.part + int64_t(blockIdx.x) * tri(a.W);
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
        if (!mine[u]) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = 16 * ti[u] + kr + 4 * q, col = 16 * tj[u] + kc;
            if (row <= col && col < a.W) out[upper_at(row, col, a.W)] = acc[u][q];
        }
    }
    if (tid == 0 && bad_rows) gae::add_count(&a.status->nonfinite_rows, bad_rows);
}

// grid (ceil(tri(W) / 16), F): fold_lists.h's reduce_entries over the chunks of fold blockIdx.y (their number is known on
// the device only)
constexpr int kReduceEntries = kWaves * gae::kWaveEntries;

__global__ __launch_bounds__(kThreads) void ridge_reduce_kernel(const StatsArgs a)
{
    const int f = blockIdx.y;
    const int64_t tw = tri(a.W), e1 = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    double *out = a.stats + int64_t(f) * tw;
    if (!gae::folds_valid(a.list)) {                                   // flagged by the stats launch
        if (e1 < tw) out[e1] = __builtin_nan("");
        return;
    }
    int lo, hi;
    const int64_t P = gae::fold_chunks(a.list, f, kChunk, lo, hi);
    gae::reduce_entries<kThreads>(a.part + gae::chunks_before(a.list, f, kChunk) * tw, P, tw,
                                  [](int64_t) { return true; }, [&](int64_t e, double s) { out[e] = s; });
}

// ------------------------------------------------------------------------------------------------------ solve
struct SolveArgs {
    const double *stats;                   // [F][tri(W)]
    int d, t, F, L, W, no_icpt;
    const float *pivot;
    const double *lambdas;
    double *coef, *icpt, *sse;
    int32_t *info;
    gae_ridge_status *status;
};

inline size_t solve_lds(int64_t d, int64_t t) { return size_t(tri(d) + 2 * t * d + d + 4 * (d + t) + t + 8) * 8; }

// one block per (model, lambda): block m L + l
__global__ __launch_bounds__(kThreads) void ridge_solve_kernel(const SolveArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int d = a.d, t = a.t, W = a.W, D = d + t, tid = threadIdx.x;
    const int l = blockIdx.x % a.L, m = blockIdx.x / a.L;
    const int64_t tw = tri(W);
    const int td = int(tri(d));
    double *Lm = lds;                      // rows 0 .. d - 1: packed lower triangle; rows d .. D - 1: [t][d], the right-hand sides
    double *dg = Lm + td + t * d;          // [d]: the factor's diagonal
    double *mu = dg + d;                   // [D]
    double *s0 = mu + D;                   // [D]: S[0, 1 + k]
    double *pv = s0 + D;                   // [D]: the pivot
    double *Wt = pv + D;                   // [t][d]: the solution
    double *bq = Wt + t * d;               // [t]: the intercept in pivoted coordinates
    double *qs = bq + t;                   // [D + 2] (W + 1 at most): terms of the quadratic form
    auto row_at = [&](int i) { return i < d ? i * (i + 1) / 2 : td + (i - d) * d; };
    // training moment (i, j), i <= j: the folds other than the model's own, ascending
    auto S_at = [&](int i, int j) {
        const double *p = a.stats + upper_at(i, j, W);
        double s = 0.0;
        for (int f = 0; f < a.F; ++f)
            if (f != m) s += p[int64_t(f) * tw];
        return s;
    };
    const int64_t cell = int64_t(m) * a.L + l;
    const double lam = a.lambdas[l];
    const double c = S_at(0, 0);
    int info = 0;
    if (!(lam >= 0.0 && lam <= DBL_MAX)) {
        info = -2;
        if (tid == 0 && m == 0) gae::or_bits(&a.status->errors, GAE_RIDGE_ERR_LAMBDA);
    } else if (!(c > 0.0)) {
        info = -1;
    }
    if (info == 0) {
        for (int k = tid; k < D; k += kThreads) {
            const double s = S_at(0, 1 + k);
            s0[k] = s;
            mu[k] = a.no_icpt ? 0.0 : s / c;
            pv[k] = a.pivot ? double(a.pivot[k]) : 0.0;
        }
        __syncthreads();
        for (int e = tid; e < td + t * d; e += kThreads) {
            int i, j;
            if (e < td) {
                i = int((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
                while (i * (i + 1) / 2 > e) --i;
                while ((i + 1) * (i + 2) / 2 <= e) ++i;
                j = e - i * (i + 1) / 2;
            } else {
                i = d + (e - td) / d;
                j = (e - td) % d;
            }
            double v = S_at(1 + j, 1 + i);                             // j <= i
            if (a.no_icpt) v += pv[i] * s0[j] + pv[j] * s0[i] + c * pv[i] * pv[j];     // moments about 0
            else v -= s0[i] * mu[j];
            if (i == j) v += lam;
            Lm[e] = v;
        }
        __syncthreads();
        // ---- Cholesky-Crout, column by column; thread r owns row j + r, the rows d .. D - 1 are the right-hand sides
        info = gae::cholesky_crout(Lm, dg, d, D, tid, row_at);
    }
    if (info == 0) {
        // ---- back substitution L^T w = z, row d - 1 first
        for (int i = d - 1; i >= 0; --i) {
            const double *ri = Lm + row_at(i);
            const double dii = dg[i];
            for (int p = tid; p < t * (i + 1); p += kThreads) {
                const int jt = p / (i + 1), k = p % (i + 1);
                double *z = Lm + row_at(d + jt);
                const double wi = z[i] / dii;
                if (k == i) Wt[jt * d + i] = wi;
                else z[k] -= ri[k] * wi;
            }
            __syncthreads();
        }
        if (tid < t) {
            const double *w = Wt + tid * d;
            double mw = 0.0, pw = 0.0;
            for (int i = 0; i < d; ++i) { mw += mu[i] * w[i]; pw += pv[i] * w[i]; }
            double b;
            if (a.no_icpt) { b = 0.0; bq[tid] = pw - pv[d + tid]; }
            else { bq[tid] = mu[d + tid] - mw; b = pv[d + tid] + mu[d + tid] - mw - pw; }
            a.icpt[cell * t + tid] = b;
        }
        for (int e = tid; e < t * d; e += kThreads) a.coef[cell * t * d + e] = Wt[e];
        __syncthreads();
        // ---- held-out SSE of fold m: u^T M_m u with u = [-b', -w, e_j], over the entries 0, 1 .. d, 1 + d + j
        if (m < a.F) {
            const double *M = a.stats + int64_t(m) * tw;
            for (int jt = 0; jt < t; ++jt) {
                const double *w = Wt + jt * d;
                auto idx = [&](int q) { return q <= d ? q : 1 + d + jt; };
                auto uu = [&](int q) { return q == 0 ? -bq[jt] : (q <= d ? -w[q - 1] : 1.0); };
                if (tid < d + 2) {
                    const int ia = idx(tid);
                    double r = 0.0;
                    for (int q = 0; q < d + 2; ++q) {
                        const int ib = idx(q);
                        r += M[ia <= ib ? upper_at(ia, ib, W) : upper_at(ib, ia, W)] * uu(q);
                    }
                    qs[tid] = uu(tid) * r;
                }
                __syncthreads();
                if (tid == 0) {
                    double s = 0.0;
                    for (int q = 0; q < d + 2; ++q) s += qs[q];
                    a.sse[cell * t + jt] = s;
                }
                __syncthreads();
            }
        }
    } else {
        const double nan = __builtin_nan("");
        for (int e = tid; e < t * d; e += kThreads) a.coef[cell * t * d + e] = nan;
        if (tid < t) {
            a.icpt[cell * t + tid] = nan;
            if (m < a.F) a.sse[cell * t + tid] = nan;
        }
    }
    if (tid == 0) a.info[cell] = info;
}

struct Plan { int64_t W, chunks, need; };

int plan(const char *fn, int64_t n_rows, int64_t d, int64_t t, int64_t folds, Plan &p)
{
    GAE_REQUIRE(d >= 1 && d <= kMaxD, GAE_E_RANGE, "%s: d = %lld outside 1..128", fn, (long long)d);
    GAE_REQUIRE(t >= 1 && t <= kMaxT, GAE_E_RANGE, "%s: t = %lld outside 1..8", fn, (long long)t);
    GAE_REQUIRE(folds >= 1 && folds <= kMaxF, GAE_E_RANGE, "%s: folds = %lld outside 1..32", fn, (long long)folds);
    GAE_REQUIRE(n_rows >= 0, GAE_E_SIZE, "%s: negative n_rows = %lld", fn, (long long)n_rows);
    GAE_REQUIRE(n_rows < (int64_t(1) << 31), GAE_E_SIZE, "%s: n_rows = %lld beyond int32 row ids", fn, (long long)n_rows);
    p.W = 1 + d + t;
    p.chunks = cdiv(n_rows, kChunk) + folds;               // every fold ends in at most one partial chunk
    p.need = up256(p.chunks * tri(p.W) * 8) + 256;
    return GAE_OK;
}

template <int NT>
int launch_stats(int64_t blocks, hipStream_t st, const StatsArgs &a)
{
    constexpr int WP = 16 * NT, pitch = gae::tile_pitch(NT);
    const size_t lds = size_t(2 * kStage * pitch + WP) * 8 + kChunk * 4 + 16;
    return gae::launch_lds<&ridge_stats_kernel<NT>>("ridge_stats_kernel", blocks, kThreads, lds, st, a);
}

} // namespace

extern "C" int64_t gae_ridge_workspace_bytes(int64_t n_rows, int64_t d, int64_t t, int64_t folds)
{
    Plan p;
    if (const int rc = plan("gae_ridge_workspace_bytes", n_rows, d, t, folds, p)) return rc;
    return p.need;
}

extern "C" int gae_ridge_stats(const float *X, int64_t ldx, const float *Y, int64_t ldy, int64_t n, int64_t d, int64_t t,
                               const float *pivot, const int32_t *rows, int64_t n_rows, const int32_t *fold_ptr,
                               int64_t folds, double *stats, gae_ridge_status *status, void *workspace,
                               int64_t workspace_bytes, void *stream)
{
    const char *fn = "gae_ridge_stats";
    Plan p;
    if (const int rc = plan(fn, n_rows, d, t, folds, p)) return rc;
    GAE_REQUIRE(n >= 0, GAE_E_SIZE, "%s: negative n = %lld", fn, (long long)n);
    GAE_REQUIRE(n < (int64_t(1) << 31), GAE_E_SIZE, "%s: n = %lld beyond int32 row ids", fn, (long long)n);
    GAE_REQUIRE(ldx >= d && ldy >= t, GAE_E_SIZE, "%s: leading dimension too small (ldx %lld < d or ldy %lld < t)", fn,
                (long long)ldx, (long long)ldy);
    GAE_REQUIRE(rows || (n_rows == n && folds == 1), GAE_E_SIZE,
                "%s: rows is NULL (rows 0 .. n - 1 in one fold) with n_rows = %lld, n = %lld, folds = %lld", fn,
                (long long)n_rows, (long long)n, (long long)folds);
    GAE_REQUIRE(!rows || fold_ptr, GAE_E_NULL, "%s: fold_ptr is NULL", fn);
    GAE_REQUIRE(n_rows == 0 || (X && Y), GAE_E_NULL, "%s: X / Y is NULL", fn);
    GAE_REQUIRE(stats && status, GAE_E_NULL, "%s: stats / status is NULL", fn);
    GAE_REQUIRE(workspace, GAE_E_NULL, "%s: workspace is NULL", fn);
    GAE_REQUIRE(workspace_bytes >= p.need, GAE_E_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn,
                (long long)workspace_bytes, (long long)p.need);

    StatsArgs a;
    a.X = X; a.Y = Y; a.ldx = ldx; a.ldy = ldy;
    a.n = int(n); a.d = int(d); a.t = int(t); a.W = int(p.W);
    a.pivot = pivot;
    a.list = gae::FoldList{rows, fold_ptr, int(folds), int(n_rows)};
    a.part = static_cast<double *>(workspace);
    a.stats = stats; a.status = status;
    hipStream_t st = gae::as_stream(stream);
    const int64_t blocks = rows ? p.chunks : cdiv(n_rows, kChunk);
    if (blocks > 0) {
        int rc = GAE_OK;
        switch (cdiv(p.W, 16)) {
        case 1: rc = launch_stats<1>(blocks, st, a); break;
        case 2: rc = launch_stats<2>(blocks, st, a); break;
        case 3: rc = launch_stats<3>(blocks, st, a); break;
        case 4: rc = launch_stats<4>(blocks, st, a); break;
        case 5: rc = launch_stats<5>(blocks, st, a); break;
        case 6: rc = launch_stats<6>(blocks, st, a); break;
        case 7: rc = launch_stats<7>(blocks, st, a); break;
        case 8: rc = launch_stats<8>(blocks, st, a); break;
        default: rc = launch_stats<9>(blocks, st, a); break;
        }
        if (rc) return rc;
    }
    hipLaunchKernelGGL(ridge_reduce_kernel, dim3(unsigned(cdiv(tri(p.W), kReduceEntries)), unsigned(folds)), dim3(kThreads), 0, st,
                       a);
    GAE_CHECK_LAUNCH("ridge_reduce_kernel");
    return GAE_OK;
}

extern "C" int gae_ridge_solve(const double *stats, int64_t d, int64_t t, int64_t folds, const float *pivot,
                               const double *lambdas, int64_t n_lambdas, int flags, double *coef, double *intercept,
                               double *cv_sse, int32_t *info, gae_ridge_status *status, void *stream)
{
    const char *fn = "gae_ridge_solve";
    Plan p;
    if (const int rc = plan(fn, 0, d, t, folds, p)) return rc;
    GAE_REQUIRE(n_lambdas >= 1 && n_lambdas <= kMaxL, GAE_E_RANGE, "%s: n_lambdas = %lld outside 1..64", fn,
                (long long)n_lambdas);
    GAE_REQUIRE((flags & ~GAE_RIDGE_NO_INTERCEPT) == 0, GAE_E_RANGE, "%s: unknown flags 0x%x", fn, flags);
    GAE_REQUIRE(stats && lambdas, GAE_E_NULL, "%s: stats / lambdas is NULL", fn);
    GAE_REQUIRE(coef && intercept && cv_sse && info && status, GAE_E_NULL,
                "%s: coef / intercept / cv_sse / info / status is NULL", fn);
    const SolveArgs a{stats, int(d), int(t), int(folds), int(n_lambdas), int(p.W), (flags & GAE_RIDGE_NO_INTERCEPT) ? 1 : 0,
                      pivot, lambdas, coef, intercept, cv_sse, info, status};
    hipStream_t st = gae::as_stream(stream);
    return gae::launch_lds<&ridge_solve_kernel>("ridge_solve_kernel", n_lambdas * (folds + 1), kThreads, solve_lds(d, t), st,
                                                a);
}
