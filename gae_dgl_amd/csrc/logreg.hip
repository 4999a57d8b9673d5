// K28: multinomial (softmax) logistic regression with an L2 penalty on frozen features, lambda by k-fold CV (ops.logreg,
// GAE.classify_nodes, GAE.logreg_graphs).  X fp32 [n, d] (ldx), y int32 [n]; 1 <= d <= 128, 2 <= c <= 32 classes,
// 1 <= F <= 32 folds, 1 <= L <= 64 lambdas.  The contract -- the objective, the majoriser, the iteration, the order of
// every sum, the state, the status block, info -- is the K28 comment of include/gae_hip_experimental.h.
//
// Model g = m L + l: fold model m < F (trains on every fold but m) or the all-rows model m = F, at lambda l.  With
// D1 = d + 1 a model's parameters are [c][D1], the intercept in column 0; a row is x~ = [1, x - p] in fp32.
//
// Launches (ordinary ones, no float atomics):
//   factor  one block per model: A = S / 2 + lambda diag(0, 1 .. 1) from gae_ridge_stats' moments (the training folds,
//           ascending), ridge's Cholesky-Crout in LDS (cholesky.h), the factor and the zeroed iteration state.
//   pass    grid (slabs, model tiles): a slab is kSlabChunks consecutive chunks of kChunk listed rows (fold_lists.h's chunk
//           order: a chunk never straddles folds), a tile kTile consecutive models of the launch.  Per chunk the block stages x~ in LDS once;
//           per model of the tile that uses the chunk: logits x~ V^T on v_mfma_f32_16x16x4_f32 (wave w owns row tile w,
//           one k-ascending chain per element) -> LDS; one thread per row: max, subtract, exp, ascending sum, one
//           reciprocal, minus the one-hot label -> LDS; gradient R^T x~ on the same instruction, its [CT][NT] output tiles
//           dealt round-robin to the waves, accumulated in registers over the slab's chunks in ascending order; one
//           partial per (slab, model).  Evaluation mode: the same products, then per row the fp64 negative log-likelihood
//           and the arg-max test, added per model in ascending row order; a second launch adds the slabs.
//   update  one block per model: the slab partials in fp64 in THE order of partial lists, + lambda D V, the c solves with
//           the stored factor in LDS, the restart test and the stopping rule in fp64, the next V in fp32.
//   predict one block per kChunk rows, the pass kernel's staging, product and softmax code.
//
// LDS (d = 128, c = 32: pitch 148, CP 32): pass 64 . 148 . 4 (x~) + 4 . 32 . 148 . 4 (V of the tile) + 64 . 33 . 4 (logits)
// + pivot, row ids, labels, flags, 64 fp64 = 121 KB, one block per CU; d = 48, c = 2: 40 KB, three (registers).  factor
// 67 KB, update 138 KB (the factor, two [c][D1] fp64 tables, the reduction scratch).
#include "common.h"
#include "cholesky.h"
#include "fold_lists.h"

namespace {

using gae::add_count;
using gae::cdiv;
using gae::mfma4;
using gae::or_bits;
using gae::tri;
using gae::upper_at;
using gae::v4f;

constexpr int kMaxD = 128, kMaxC = 32, kMaxF = 32, kMaxL = 64;
constexpr int kChunk = GAE_LOGREG_CHUNK_ROWS;
constexpr int kSlabChunks = GAE_LOGREG_SLAB_CHUNKS;
constexpr int kTile = 4;                   // models per block of the pass
constexpr int kThreads = 256, kWaves = kThreads / gae::kWave;
static_assert(kChunk == 16 * kWaves, "the logits of a chunk: one row tile per wave");

// ------------------------------------------------------------------------------------------------------ shapes, state
struct Shape {
    int d, c, D1, NT, WP, pitch, CT, CP, zp, KS, cD;
};

__host__ __device__ inline Shape shape_of(int d, int c)
{
    Shape s;
    s.d = d; s.c = c; s.D1 = d + 1;
    s.NT = (s.D1 + 15) / 16; s.WP = 16 * s.NT; s.pitch = s.WP + 4;      // pitch % 32 is 4 or 20: the 16 rows of an operand
    s.CT = (c + 15) / 16; s.CP = 16 * s.CT; s.zp = s.CP + 1;           // ... read start in different banks
    s.KS = (s.D1 + 3) / 4;
    s.cD = c * s.D1;
    return s;
}

struct Plan { int64_t models, chunks, slabs, batch, need; };

// the workspace: the models' state, then one launch's partials
struct Layout {
    double *factor;                        // [models][tri(D1)]: packed lower triangle, the factor's diagonal in place
    double *W, *Wprev;                     // [models][c][D1]
    double *t;                             // [models]
    float *V;                              // [models][c][D1]: where the next pass evaluates; after the fit fp32(W)
    int32_t *active, *ok;                  // [models]
    float *part;                           // [slabs][batch][c][D1]
    double *enll;                          // [slabs][batch]
    int64_t *ecorrect;                     // [slabs][batch]
};

Layout carve(gae::Carver &cv, const Plan &p, const Shape &s)
{
    Layout l;
    l.factor = cv.take<double>(p.models * tri(s.D1));
    l.W = cv.take<double>(p.models * s.cD);
    l.Wprev = cv.take<double>(p.models * s.cD);
    l.t = cv.take<double>(p.models);
    l.V = cv.take<float>(p.models * s.cD);
    l.active = cv.take<int32_t>(p.models);
    l.ok = cv.take<int32_t>(p.models);
    l.part = cv.take<float>(p.slabs * p.batch * s.cD);
    l.enll = cv.take<double>(p.slabs * p.batch);
    l.ecorrect = cv.take<int64_t>(p.slabs * p.batch);
    return l;
}

int plan(const char *fn, int64_t n_rows, int64_t d, int64_t c, int64_t folds, int64_t n_lambdas, int64_t batch, Plan &p)
{
    GAE_REQUIRE(d >= 1 && d <= kMaxD, GAE_E_RANGE, "%s: d = %lld outside 1..128", fn, (long long)d);
    GAE_REQUIRE(c >= 2 && c <= kMaxC, GAE_E_RANGE, "%s: c = %lld outside 2..32", fn, (long long)c);
    GAE_REQUIRE(folds >= 1 && folds <= kMaxF, GAE_E_RANGE, "%s: folds = %lld outside 1..32", fn, (long long)folds);
    GAE_REQUIRE(n_lambdas >= 1 && n_lambdas <= kMaxL, GAE_E_RANGE, "%s: n_lambdas = %lld outside 1..64", fn,
                (long long)n_lambdas);
    p.models = (folds + 1) * n_lambdas;
    GAE_REQUIRE(batch >= 1 && batch <= p.models, GAE_E_RANGE, "%s: model_batch = %lld outside 1..%lld", fn, (long long)batch,
                (long long)p.models);
    GAE_REQUIRE(n_rows >= 0, GAE_E_SIZE, "%s: negative n_rows = %lld", fn, (long long)n_rows);
    GAE_REQUIRE(n_rows < (int64_t(1) << 31), GAE_E_SIZE, "%s: n_rows = %lld beyond int32 row ids", fn, (long long)n_rows);
    p.chunks = cdiv(n_rows, kChunk) + folds;               // every fold ends in at most one partial chunk
    p.slabs = cdiv(p.chunks, kSlabChunks);
    p.batch = batch;
    gae::Carver cv(nullptr);
    carve(cv, p, shape_of(int(d), int(c)));
    p.need = cv.bytes();
    return GAE_OK;
}

int range_ok(const char *fn, const Plan &p, int64_t model_lo, int64_t model_count)
{
    GAE_REQUIRE(model_lo >= 0 && model_count >= 1 && model_count <= p.batch && model_lo + model_count <= p.models, GAE_E_RANGE,
                "%s: models %lld .. %lld + %lld outside the %lld models or beyond model_batch = %lld", fn, (long long)model_lo,
                (long long)model_lo, (long long)model_count, (long long)p.models, (long long)p.batch);
    return GAE_OK;
}

// ------------------------------------------------------------------------------------------------------ factor
struct FactorArgs {
    const double *stats;                   // gae_ridge_stats with t = 1: [F][tri(d + 2)]
    int d, c, F, L;
    const double *lambdas;
    Layout lay;
    double *coef, *icpt;
    int32_t *info, *n_iter, *converged;
    gae_logreg_status *status;
};

__global__ __launch_bounds__(kThreads) void logreg_factor_kernel(const FactorArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const int D1 = a.d + 1, Ws = a.d + 2, tid = threadIdx.x;
    const int g = blockIdx.x, m = g / a.L, l = g % a.L;
    const int td = int(tri(D1)), cD = a.c * D1;
    const int64_t tws = tri(Ws);
    double *Lm = ldsd;                     // packed lower triangle
    double *dg = Lm + td;                  // [D1]
    auto row_at = [&](int i) { return i * (i + 1) / 2; };
    auto S_at = [&](int i, int j) {        // training moment (i, j), i <= j: the folds other than the model's, ascending
        const double *p = a.stats + upper_at(i, j, Ws);
        double s = 0.0;
        for (int f = 0; f < a.F; ++f)
            if (f != m) s += p[int64_t(f) * tws];
        return s;
    };
    const double lam = a.lambdas[l];
    int info = 0;
    if (!(lam >= 0.0 && lam <= DBL_MAX)) {
        info = -2;
        if (tid == 0 && m == 0) or_bits(&a.status->errors, GAE_LOGREG_ERR_LAMBDA);
    } else if (!(S_at(0, 0) > 0.0)) {
        info = -1;
    }
    if (info == 0) {
        for (int e = tid; e < td; e += kThreads) {
            int i = int((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
            while (i * (i + 1) / 2 > e) --i;
            while ((i + 1) * (i + 2) / 2 <= e) ++i;
            const int j = e - i * (i + 1) / 2;
            double v = 0.5 * S_at(j, i);                               // j <= i
            if (i == j && i >= 1) v += lam;
            Lm[e] = v;
        }
        __syncthreads();
        info = gae::cholesky_crout(Lm, dg, D1, D1, tid, row_at);
    }
    double *fo = a.lay.factor + int64_t(g) * td;
    if (info == 0) {
        for (int e = tid; e < td; e += kThreads) fo[e] = Lm[e];
        __syncthreads();
        for (int i = tid; i < D1; i += kThreads) fo[row_at(i) + i] = dg[i];
    }
    const double init = info == 0 ? 0.0 : __builtin_nan("");
    for (int e = tid; e < cD; e += kThreads) {
        a.lay.W[int64_t(g) * cD + e] = 0.0;
        a.lay.Wprev[int64_t(g) * cD + e] = 0.0;
        a.lay.V[int64_t(g) * cD + e] = 0.f;
    }
    for (int e = tid; e < a.c * a.d; e += kThreads) a.coef[int64_t(g) * a.c * a.d + e] = init;
    if (tid < a.c) a.icpt[int64_t(g) * a.c + tid] = init;
    if (tid == 0) {
        a.lay.t[g] = 1.0;
        a.lay.active[g] = info == 0;
        a.lay.ok[g] = info == 0;
        a.info[g] = info;
        a.n_iter[g] = 0;
        a.converged[g] = 0;
        if (info == 0) add_count(&a.status->active_models, 1);
    }
}

// ------------------------------------------------------------------------------------------------------ pass
struct PassArgs {
    const float *X;
    int64_t ldx;
    const int32_t *y;
    int n, d, c, L;
    const float *pivot;                    // [d] or NULL
    gae::FoldList list;                    // the listed rows (fold_lists.h)
    int model_lo, model_count, eval;
    Layout lay;
    gae_logreg_status *status;
};

// rows lo .. lo + nrows - 1 of a list (rows == NULL: the ids themselves) as x~ = [1, x - p, 0 ...] in Xa[kChunk][pitch], zero
// rows past nrows and for ids outside [0, n); rid[] the ids (-1: no row); bad[] != 0: the row holds a non-finite value.
// rid and bad are in place after the caller's next barrier; bad[] is zeroed before the previous one.
__device__ __forceinline__ bool stage_rows(const Shape &s, const float *__restrict__ X, int64_t ldx, int n,
                                           const gae::FoldList &list, int64_t lo, int nrows, const float *pv, float *Xa,
                                           int *rid, int *bad, int tid)
{
    bool bad_id = false;
    for (int e = tid; e < kChunk * s.WP; e += kThreads) {
        const int r = e / s.WP, col = e - r * s.WP;
        const int id = r < nrows ? gae::row_id(list, lo + r, n, bad_id) : -1;
        float v = 0.f;
        if (id >= 0) {
            if (col == 0) v = 1.f;
            else if (col <= s.d) {
                const float x = X[int64_t(id) * ldx + (col - 1)];
                if (!gae::finite32(x)) atomicOr(&bad[r], 1);
                v = x - pv[col];                                       // one rounded subtraction
            }
        }
        Xa[r * s.pitch + col] = v;
        if (col == 0) rid[r] = id;
    }
    return bad_id;
}

// the logits of the chunk for one model: wave w owns rows 16 w .. 16 w + 15; Zs[row][class] for every class tile
__device__ __forceinline__ void logits_to_lds(const Shape &s, const float *Xa, const float *Vs, float *Zs, int wave, int lane)
{
    const int l15 = lane & 15, g4 = lane >> 4;
    const float *ap = Xa + (16 * wave + l15) * s.pitch + g4;
    for (int ct = 0; ct < s.CT; ++ct) {
        const float *bp = Vs + (16 * ct + l15) * s.pitch + g4;
        v4f z = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < s.KS; ++k) z = mfma4(ap[4 * k], bp[4 * k], z);
#pragma unroll
        for (int q = 0; q < 4; ++q) Zs[(16 * wave + 4 * g4 + q) * s.zp + 16 * ct + l15] = z[q];
    }
}

// one row's softmax in fp32, in place: max, subtract, exp, ascending sum, one reciprocal
__device__ __forceinline__ void softmax_row(float *z, int c)
{
    float mx = z[0];
    for (int k = 1; k < c; ++k) mx = fmaxf(mx, z[k]);
    float sm = 0.f;
    for (int k = 0; k < c; ++k) {
        const float e = expf(z[k] - mx);
        z[k] = e;
        sm += e;
    }
    const float inv = 1.f / sm;
    for (int k = 0; k < c; ++k) z[k] *= inv;
}

inline size_t pass_lds(const Shape &s, int tile)
{
    return size_t(kChunk) * 8 + size_t(kChunk * s.pitch + tile * s.CP * s.pitch + kChunk * s.zp + s.WP) * 4 + size_t(4 * kChunk) * 4;
}

template <int TPW>
__global__ __launch_bounds__(kThreads) void logreg_pass_kernel(const PassArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const Shape s = shape_of(a.d, a.c);
    double *rowd = ldsd;                                               // [kChunk]: a row's negative log-likelihood
    float *Xa = reinterpret_cast<float *>(rowd + kChunk);              // [kChunk][pitch]
    float *Vs = Xa + kChunk * s.pitch;                                 // [kTile][CP][pitch]
    float *Zs = Vs + kTile * s.CP * s.pitch;                           // [kChunk][zp]
    float *pv = Zs + kChunk * s.zp;                                    // [WP]: 0, p, 0 ...
    int *rid = reinterpret_cast<int *>(pv + s.WP);                     // [kChunk]
    int *lab = rid + kChunk, *bad = lab + kChunk, *hit = bad + kChunk; // [kChunk] each
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, g4 = lane >> 4;
    const int slab = blockIdx.x, Mb = a.model_count;

    int gm[kTile], mm[kTile];
    bool on[kTile];
    bool any = false;
#pragma unroll
    for (int mi = 0; mi < kTile; ++mi) {
        const int local = blockIdx.y * kTile + mi;
        gm[mi] = a.model_lo + local;
        on[mi] = local < Mb && (a.eval ? a.lay.ok[gm[mi]] : a.lay.active[gm[mi]]) != 0;
        mm[mi] = gm[mi] / a.L;
        any = any || on[mi];
    }
    if (!any) return;                                                  // frozen models: the block exits at once
    if (!gae::folds_valid(a.list)) {
        if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) or_bits(&a.status->errors, GAE_LOGREG_ERR_FOLD_PTR);
        return;
    }
#pragma unroll
    for (int mi = 0; mi < kTile; ++mi) {
        if (!on[mi]) continue;
        const float *V = a.lay.V + int64_t(gm[mi]) * s.cD;
        float *dst = Vs + mi * s.CP * s.pitch;
        for (int e = tid; e < s.CP * s.pitch; e += kThreads) {
            const int k = e / s.pitch, j = e - k * s.pitch;
            dst[e] = (k < s.c && j < s.D1) ? V[k * s.D1 + j] : 0.f;
        }
    }
    for (int col = tid; col < s.WP; col += kThreads) pv[col] = (a.pivot && col >= 1 && col <= s.d) ? a.pivot[col - 1] : 0.f;
    if (tid < kChunk) bad[tid] = 0;

    v4f acc[kTile][TPW];
#pragma unroll
    for (int mi = 0; mi < kTile; ++mi)
#pragma unroll
        for (int u = 0; u < TPW; ++u) acc[mi][u] = v4f{0.f, 0.f, 0.f, 0.f};
    double nll[kTile] = {0.0, 0.0, 0.0, 0.0};                         // thread 0
    long long cor[kTile] = {0, 0, 0, 0};
    bool bad_id = false, bad_label = false;

    for (int q = 0; q < kSlabChunks; ++q) {
        const gae::Chunk ch = gae::chunk_of(a.list, int64_t(slab) * kSlabChunks + q, kChunk);
        if (ch.fold < 0) break;                                        // past the last chunk
        const int fold = ch.fold, lo = ch.lo, hi = ch.hi;
        bool use[kTile];
        bool used = false;
#pragma unroll
        for (int mi = 0; mi < kTile; ++mi) {                           // a chunk of fold f is not part of model f's training set:
            use[mi] = on[mi] && (a.eval ? (mm[mi] == fold || mm[mi] == a.list.F) : mm[mi] != fold);     // skipped, not masked
            used = used || use[mi];
        }
        if (!used) continue;
        const int nrows = hi - lo;
        __syncthreads();                                               // the previous chunk is consumed; pv, Vs, bad are in place
        bad_id = stage_rows(s, a.X, a.ldx, a.n, a.list, lo, nrows, pv, Xa, rid, bad, tid) || bad_id;
        __syncthreads();
        if (tid < kChunk) {
            int yy = -1;
            if (rid[tid] >= 0) {
                yy = a.y[rid[tid]];
                if (unsigned(yy) >= unsigned(s.c)) { bad_label = true; yy = -1; }
            }
            lab[tid] = yy;
        }
#pragma unroll
        for (int mi = 0; mi < kTile; ++mi) {
            if (!use[mi]) continue;                                    // the same in every thread
            logits_to_lds(s, Xa, Vs + mi * s.CP * s.pitch, Zs, wave, lane);
            __syncthreads();
            if (tid < kChunk) {
                float *z = Zs + tid * s.zp;
                const int yy = lab[tid];
                if (rid[tid] < 0) {
                    for (int k = 0; k < s.c; ++k) z[k] = 0.f;
                    rowd[tid] = 0.0;
                    hit[tid] = 0;
                } else if (!a.eval) {
                    softmax_row(z, s.c);
                    if (yy >= 0) z[yy] -= 1.f;                         // the residual: minus the one-hot label
                } else {
                    float mx = z[0];
                    int arg = 0;
                    for (int k = 1; k < s.c; ++k)
                        if (z[k] > mx) { mx = z[k]; arg = k; }         // ties go to the lower class
                    double sm = 0.0;
                    for (int k = 0; k < s.c; ++k) sm += exp(double(z[k] - mx));
                    rowd[tid] = yy >= 0 ? log(sm) - double(z[yy] - mx) : 0.0;
                    hit[tid] = yy >= 0 && arg == yy;
                }
            }
            __syncthreads();
            if (!a.eval) {
#pragma unroll
                for (int u = 0; u < TPW; ++u) {
                    const int e = wave + kWaves * u;
                    if (e >= s.CT * s.NT) continue;                    // the same in every lane of the wave
                    const int ct = e / s.NT, nt = e - ct * s.NT;
                    const float *ap = Zs + g4 * s.zp + 16 * ct + l15, *bp = Xa + g4 * s.pitch + 16 * nt + l15;
                    v4f g = acc[mi][u];
                    for (int k = 0; k < kChunk / 4; ++k) g = mfma4(ap[4 * k * s.zp], bp[4 * k * s.pitch], g);
                    acc[mi][u] = g;
                }
            } else if (tid == 0) {
                double t = 0.0;
                int h = 0;
                for (int r = 0; r < nrows; ++r) { t += rowd[r]; h += hit[r]; }
                nll[mi] += t;
                cor[mi] += h;
            }
            __syncthreads();                                           // Zs is free for the next model
        }
    }
    if (bad_id) or_bits(&a.status->errors, GAE_LOGREG_ERR_ROW_ID);
    if (bad_label) or_bits(&a.status->errors, GAE_LOGREG_ERR_LABEL);

#pragma unroll
    for (int mi = 0; mi < kTile; ++mi) {
        if (!on[mi]) continue;
        const int64_t cell = int64_t(slab) * Mb + (blockIdx.y * kTile + mi);
        if (a.eval) {
            if (tid == 0) { a.lay.enll[cell] = nll[mi]; a.lay.ecorrect[cell] = cor[mi]; }
            continue;
        }
        float *out = a.lay.part + cell * s.cD;
#pragma unroll
        for (int u = 0; u < TPW; ++u) {
            const int e = wave + kWaves * u;
            if (e >= s.CT * s.NT) continue;
            const int ct = e / s.NT, nt = e - ct * s.NT, col = 16 * nt + l15;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = 16 * ct + 4 * g4 + r;
                if (k < s.c && col < s.D1) out[k * s.D1 + col] = acc[mi][u][r];
            }
        }
    }
}

// the slabs of an evaluation pass, per model: fp64 in THE order of partial lists; the counts are integers
struct EvalArgs {
    Layout lay;
    int model_lo, model_count;
    int64_t slabs;
    double *nll;
    int64_t *correct;
};

__global__ __launch_bounds__(64) void logreg_eval_reduce_kernel(const EvalArgs a)
{
    const int local = blockIdx.x, g = a.model_lo + local, lane = threadIdx.x;
    if (!a.lay.ok[g]) {
        if (lane == 0) { a.nll[g] = __builtin_nan(""); a.correct[g] = 0; }
        return;
    }
    const int L = gae::partial_lanes(a.slabs);
    if (L == 1 && lane > 0) return;
    const double v = gae::sum_partials<double>(a.lay.enll + local, a.slabs, a.model_count, lane, L);
    long long h = 0;
    for (int64_t q = lane; q < a.slabs; q += L) h += a.lay.ecorrect[q * a.model_count + local];
    if (L == 64) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) h += __shfl_down(h, off, 64);
    }
    if (lane == 0) { a.nll[g] = v; a.correct[g] = h; }
}

// ------------------------------------------------------------------------------------------------------ update
struct UpdateArgs {
    int d, c, L;
    const double *lambdas;
    int model_lo, model_count;
    int64_t slabs;
    int iteration, max_iter;
    double tol;
    const float *pivot;
    Layout lay;
    double *coef, *icpt;
    int32_t *info, *n_iter, *converged;
    gae_logreg_status *status;
};

inline size_t update_lds(const Shape &s) { return size_t(tri(s.D1) + 2 * s.cD + 4 * kThreads) * 8; }

// a block-wide reduction in a fixed order: thread t's value to red[t], then the tree 128, 64 .. 1
template <class Op>
__device__ __forceinline__ double block_reduce(double v, double *red, int tid, Op op)
{
    red[tid] = v;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] = op(red[tid], red[tid + off]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kThreads) void logreg_update_kernel(const UpdateArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const Shape s = shape_of(a.d, a.c);
    const int D1 = s.D1, cD = s.cD, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int local = blockIdx.x, g = a.model_lo + local;
    if (!a.lay.active[g]) return;                                      // a finished model is frozen
    const int td = int(tri(D1));
    double *Lf = ldsd;                     // the factor
    double *G = Lf + td;                   // [c][D1]: the gradient
    double *Z = G + cD;                    // [c][D1]: the right-hand sides, then the solution
    double *red = Z + cD;                  // [kThreads]
    auto row_at = [&](int i) { return i * (i + 1) / 2; };
    const double lam = a.lambdas[g % a.L];
    const double *fi = a.lay.factor + int64_t(g) * td;
    const float *V = a.lay.V + int64_t(g) * cD;
    double *W = a.lay.W + int64_t(g) * cD, *Wp = a.lay.Wprev + int64_t(g) * cD;
    for (int e = tid; e < td; e += kThreads) Lf[e] = fi[e];
    // ---- G = the slab partials in fp64, slabs ascending in the order of partial lists, + lambda D V
    const float *p0 = a.lay.part + int64_t(local) * cD;
    const int64_t stride = int64_t(a.model_count) * cD;
    if (gae::partial_lanes(a.slabs) == 1) {
        for (int e = tid; e < cD; e += kThreads) G[e] = gae::sum_partials<double>(p0 + e, a.slabs, stride, 0, 1);
    } else {
        for (int e = wave; e < cD; e += kWaves) {                      // all 64 lanes of the wave call
            const double v = gae::sum_partials<double>(p0 + e, a.slabs, stride, lane, 64);
            if (lane == 0) G[e] = v;
        }
    }
    __syncthreads();
    for (int e = tid; e < cD; e += kThreads) {
        const int j = e % D1;
        const double v = G[e] + (j >= 1 ? lam * double(V[e]) : 0.0);
        G[e] = v;
        Z[e] = v;
    }
    __syncthreads();
    // ---- L y = g for the c right-hand sides, column by column; Z[k][j] is final after step j - 1 and divided at the end
    for (int j = 0; j < D1 - 1; ++j) {
        const int len = D1 - 1 - j;
        const double ljj = Lf[row_at(j) + j];
        for (int p = tid; p < s.c * len; p += kThreads) {
            const int k = p / len, i = j + 1 + p - k * len;
            Z[k * D1 + i] -= Lf[row_at(i) + j] * (Z[k * D1 + j] / ljj);
        }
        __syncthreads();
    }
    for (int e = tid; e < cD; e += kThreads) Z[e] /= Lf[row_at(e % D1) + e % D1];
    __syncthreads();
    // ---- L^T x = y, row D1 - 1 first; Z[k][i] is final after step i + 1
    for (int i = D1 - 1; i >= 1; --i) {
        const double lii = Lf[row_at(i) + i];
        const double *ri = Lf + row_at(i);
        for (int p = tid; p < s.c * i; p += kThreads) {
            const int k = p / i, j = p - k * i;
            Z[k * D1 + j] -= ri[j] * (Z[k * D1 + i] / lii);
        }
        __syncthreads();
    }
    for (int e = tid; e < cD; e += kThreads) Z[e] /= Lf[row_at(e % D1) + e % D1];
    __syncthreads();
    // ---- W_new = V - A^-1 G; the step's size, the restart test <G, W_new - W>, all in fp64 in a fixed order
    double dmax = 0.0, wmax = 0.0, ip = 0.0, fin = 0.0;
    for (int e = tid; e < cD; e += kThreads) {
        const double dv = -Z[e], wn = double(V[e]) + dv;
        Z[e] = wn;
        dmax = fmax(dmax, fabs(dv));
        wmax = fmax(wmax, fabs(wn));
        ip += G[e] * (wn - W[e]);
        if (!(fabs(wn) <= DBL_MAX && fabs(G[e]) <= DBL_MAX)) fin = 1.0;
    }
    auto mx = [](double x, double y) { return fmax(x, y); };
    auto add = [](double x, double y) { return x + y; };
    dmax = block_reduce(dmax, red, tid, mx);
    wmax = block_reduce(wmax, red, tid, mx);
    ip = block_reduce(ip, red, tid, add);
    fin = block_reduce(fin, red, tid, mx);
    double *coef = a.coef + int64_t(g) * a.c * a.d, *icpt = a.icpt + int64_t(g) * a.c;
    if (fin != 0.0) {                                                  // a non-finite gradient or iterate: the model fails
        const double nan = __builtin_nan("");
        for (int e = tid; e < a.c * a.d; e += kThreads) coef[e] = nan;
        if (tid < a.c) icpt[tid] = nan;
        if (tid == 0) {
            a.info[g] = -3;
            a.n_iter[g] = a.iteration;
            a.lay.active[g] = 0;
            a.lay.ok[g] = 0;
            or_bits(&a.status->errors, GAE_LOGREG_ERR_NONFINITE);
            add_count(&a.status->active_models, -1);
        }
        return;
    }
    const bool done = dmax <= a.tol * fmax(1.0, wmax);
    const bool stop = done || a.iteration >= a.max_iter;
    const double t = a.lay.t[g];
    const double t1 = (1.0 + sqrt(1.0 + 4.0 * t * t)) * 0.5;           // the t' this pass's V was formed with
    const double tn = ip > 0.0 ? 1.0 : t1;                             // gradient restart
    const double t2 = (1.0 + sqrt(1.0 + 4.0 * tn * tn)) * 0.5;
    const double beta = stop ? 0.0 : (tn - 1.0) / t2;
    __syncthreads();                                                   // every thread has read t
    for (int e = tid; e < cD; e += kThreads) {
        const double w = W[e], wn = Z[e];
        Wp[e] = w;
        W[e] = wn;
        a.lay.V[int64_t(g) * cD + e] = float(wn + beta * (wn - w));    // stopped: fp32(W), what the evaluation reads
    }
    if (stop) {
        // the model in the caller's coordinates: x~ = x - p, so b = W[k][0] - sum_j p_j W[k][1 + j], j ascending
        for (int e = tid; e < a.c * a.d; e += kThreads) coef[e] = Z[(e / a.d) * D1 + 1 + e % a.d];
        if (tid < a.c) {
            double b = Z[tid * D1];
            if (a.pivot)
                for (int j = 0; j < a.d; ++j) b -= double(a.pivot[j]) * Z[tid * D1 + 1 + j];
            icpt[tid] = b;
        }
    }
    if (tid == 0) {
        a.lay.t[g] = tn;
        a.n_iter[g] = a.iteration;
        if (stop) {
            a.converged[g] = done;
            a.lay.active[g] = 0;
            add_count(&a.status->active_models, -1);
        }
    }
}

// ------------------------------------------------------------------------------------------------------ predict
struct PredictArgs {
    const float *X;
    int64_t ldx;
    int n, d, c;
    const double *coef, *icpt;
    const float *pivot;
    int32_t *labels;
    float *proba;
    int64_t ldp;
    gae_logreg_status *status;
};

__global__ __launch_bounds__(kThreads) void logreg_predict_kernel(const PredictArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double ldsd[];
    const Shape s = shape_of(a.d, a.c);
    float *Xa = reinterpret_cast<float *>(ldsd + kChunk);
    float *Vs = Xa + kChunk * s.pitch;                                 // [CP][pitch]
    float *Zs = Vs + s.CP * s.pitch;
    float *pv = Zs + kChunk * s.zp;
    int *rid = reinterpret_cast<int *>(pv + s.WP);
    int *bad = rid + 2 * kChunk;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t lo = int64_t(blockIdx.x) * kChunk;
    const int nrows = a.n - lo > kChunk ? kChunk : int(a.n - lo);
    for (int col = tid; col < s.WP; col += kThreads) pv[col] = (a.pivot && col >= 1 && col <= s.d) ? a.pivot[col - 1] : 0.f;
    if (tid < kChunk) bad[tid] = 0;
    // V = [b + p . w, w] in fp32: the model about the pivot
    for (int e = tid; e < s.CP * s.pitch; e += kThreads) {
        const int k = e / s.pitch, j = e - k * s.pitch;
        float v = 0.f;
        if (k < s.c && j >= 1 && j <= s.d) v = float(a.coef[k * s.d + j - 1]);
        else if (k < s.c && j == 0) {
            double b = a.icpt[k];
            if (a.pivot)
                for (int i = 0; i < s.d; ++i) b += double(a.pivot[i]) * a.coef[k * s.d + i];
            v = float(b);
        }
        Vs[e] = v;
    }
    __syncthreads();
    stage_rows(s, a.X, a.ldx, a.n, gae::FoldList{}, lo, nrows, pv, Xa, rid, bad, tid);
    __syncthreads();
    logits_to_lds(s, Xa, Vs, Zs, wave, lane);
    __syncthreads();
    if (tid < nrows) {
        float *z = Zs + tid * s.zp;
        const int64_t row = lo + tid;
        if (bad[tid]) {
            a.labels[row] = -1;
            if (a.proba)
                for (int k = 0; k < s.c; ++k) a.proba[row * a.ldp + k] = __builtin_nanf("");
            add_count(&a.status->nonfinite_rows, 1);
        } else {
            float mx = z[0];
            int arg = 0;
            for (int k = 1; k < s.c; ++k)
                if (z[k] > mx) { mx = z[k]; arg = k; }                 // ties go to the lower class
            a.labels[row] = arg;
            if (a.proba) {
                softmax_row(z, s.c);
                for (int k = 0; k < s.c; ++k) a.proba[row * a.ldp + k] = z[k];
            }
        }
    }
}

template <int TPW>
int launch_pass(int64_t slabs, int64_t tiles, size_t lds, hipStream_t st, const PassArgs &a)
{
    static int configured[16] = {0};
    int dev = 0;
    GAE_HIP(hipGetDevice(&dev));
    if (lds > 48 * 1024 && (dev < 0 || dev >= 16 || configured[dev] < int(lds))) {
        GAE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&logreg_pass_kernel<TPW>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
        if (dev >= 0 && dev < 16) configured[dev] = int(lds);
    }
    hipLaunchKernelGGL(logreg_pass_kernel<TPW>, dim3(unsigned(slabs), unsigned(tiles)), dim3(kThreads), lds, st, a);
    GAE_CHECK_LAUNCH("logreg_pass_kernel");
    return GAE_OK;
}

} // namespace

extern "C" int64_t gae_logreg_workspace_bytes(int64_t n_rows, int64_t d, int64_t c, int64_t folds, int64_t n_lambdas,
                                              int64_t model_batch)
{
    Plan p;
    if (const int rc = plan("gae_logreg_workspace_bytes", n_rows, d, c, folds, n_lambdas, model_batch, p)) return rc;
    return p.need;
}

extern "C" int gae_logreg_factor(const double *stats, int64_t d, int64_t c, int64_t folds, const double *lambdas,
                                 int64_t n_lambdas, int64_t n_rows, int64_t model_batch, double *coef, double *intercept,
                                 int32_t *info, int32_t *n_iter, int32_t *converged, gae_logreg_status *status,
                                 void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "gae_logreg_factor";
    Plan p;
    if (const int rc = plan(fn, n_rows, d, c, folds, n_lambdas, model_batch, p)) return rc;
    GAE_REQUIRE(stats && lambdas, GAE_E_NULL, "%s: stats / lambdas is NULL", fn);
    GAE_REQUIRE(coef && intercept && info && n_iter && converged && status, GAE_E_NULL,
                "%s: coef / intercept / info / n_iter / converged / status is NULL", fn);
    GAE_REQUIRE(workspace, GAE_E_NULL, "%s: workspace is NULL", fn);
    GAE_REQUIRE(workspace_bytes >= p.need, GAE_E_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn,
                (long long)workspace_bytes, (long long)p.need);
    const Shape s = shape_of(int(d), int(c));
    gae::Carver cv(workspace);
    FactorArgs a;
    a.stats = stats; a.d = int(d); a.c = int(c); a.F = int(folds); a.L = int(n_lambdas); a.lambdas = lambdas;
    a.lay = carve(cv, p, s);
    a.coef = coef; a.icpt = intercept; a.info = info; a.n_iter = n_iter; a.converged = converged; a.status = status;
    return gae::launch_lds<&logreg_factor_kernel>("logreg_factor_kernel", p.models, kThreads, size_t(tri(s.D1) + s.D1) * 8,
                                                  gae::as_stream(stream), a);
}

extern "C" int gae_logreg_pass(const float *X, int64_t ldx, const int32_t *y, int64_t n, int64_t d, int64_t c,
                               const float *pivot, const int32_t *rows, int64_t n_rows, const int32_t *fold_ptr,
                               int64_t folds, int64_t n_lambdas, int64_t model_batch, int64_t model_lo, int64_t model_count,
                               int flags, double *nll, int64_t *correct, gae_logreg_status *status, void *workspace,
                               int64_t workspace_bytes, void *stream)
{
    const char *fn = "gae_logreg_pass";
    Plan p;
    if (const int rc = plan(fn, n_rows, d, c, folds, n_lambdas, model_batch, p)) return rc;
    if (const int rc = range_ok(fn, p, model_lo, model_count)) return rc;
    GAE_REQUIRE((flags & ~GAE_LOGREG_EVAL) == 0, GAE_E_RANGE, "%s: unknown flags 0x%x", fn, flags);
    GAE_REQUIRE(n >= 0, GAE_E_SIZE, "%s: negative n = %lld", fn, (long long)n);
    GAE_REQUIRE(n < (int64_t(1) << 31), GAE_E_SIZE, "%s: n = %lld beyond int32 row ids", fn, (long long)n);
    GAE_REQUIRE(ldx >= d, GAE_E_SIZE, "%s: leading dimension too small (ldx %lld < d)", fn, (long long)ldx);
    GAE_REQUIRE(rows && fold_ptr, GAE_E_NULL, "%s: rows / fold_ptr is NULL", fn);
    GAE_REQUIRE(n_rows == 0 || (X && y), GAE_E_NULL, "%s: X / y is NULL", fn);
    const bool eval = (flags & GAE_LOGREG_EVAL) != 0;
    GAE_REQUIRE(!eval || (nll && correct), GAE_E_NULL, "%s: nll / correct is NULL in evaluation mode", fn);
    GAE_REQUIRE(status, GAE_E_NULL, "%s: status is NULL", fn);
    GAE_REQUIRE(workspace, GAE_E_NULL, "%s: workspace is NULL", fn);
    GAE_REQUIRE(workspace_bytes >= p.need, GAE_E_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn,
                (long long)workspace_bytes, (long long)p.need);
    const Shape s = shape_of(int(d), int(c));
    gae::Carver cv(workspace);
    PassArgs a;
    a.X = X; a.ldx = ldx; a.y = y;
    a.n = int(n); a.d = int(d); a.c = int(c); a.L = int(n_lambdas);
    a.pivot = pivot;
    a.list = gae::FoldList{rows, fold_ptr, int(folds), int(n_rows)};
    a.model_lo = int(model_lo); a.model_count = int(model_count); a.eval = eval ? 1 : 0;
    a.lay = carve(cv, p, s);
    a.status = status;
    hipStream_t st = gae::as_stream(stream);
    const int64_t tiles = cdiv(model_count, kTile);
    const size_t lds = pass_lds(s, kTile);
    int rc = GAE_OK;
    switch (cdiv(s.CT * s.NT, kWaves)) {                                // gradient tiles per wave
    case 1: rc = launch_pass<1>(p.slabs, tiles, lds, st, a); break;
    case 2: rc = launch_pass<2>(p.slabs, tiles, lds, st, a); break;
    case 3: rc = launch_pass<3>(p.slabs, tiles, lds, st, a); break;
    case 4: rc = launch_pass<4>(p.slabs, tiles, lds, st, a); break;
    default: rc = launch_pass<5>(p.slabs, tiles, lds, st, a); break;
    }
    if (rc || !eval) return rc;
    const EvalArgs e{a.lay, int(model_lo), int(model_count), p.slabs, nll, correct};
    hipLaunchKernelGGL(logreg_eval_reduce_kernel, dim3(unsigned(model_count)), dim3(64), 0, st, e);
    GAE_CHECK_LAUNCH("logreg_eval_reduce_kernel");
    return GAE_OK;
}

extern "C" int gae_logreg_update(int64_t d, int64_t c, int64_t folds, const double *lambdas, int64_t n_lambdas,
                                 int64_t n_rows, int64_t model_batch, int64_t model_lo, int64_t model_count,
                                 int64_t iteration, int64_t max_iter, double tol, const float *pivot, double *coef,
                                 double *intercept, int32_t *info, int32_t *n_iter, int32_t *converged,
                                 gae_logreg_status *status, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "gae_logreg_update";
    Plan p;
    if (const int rc = plan(fn, n_rows, d, c, folds, n_lambdas, model_batch, p)) return rc;
    if (const int rc = range_ok(fn, p, model_lo, model_count)) return rc;
    GAE_REQUIRE(iteration >= 1 && max_iter >= iteration && max_iter < (int64_t(1) << 31), GAE_E_RANGE,
                "%s: iteration = %lld outside 1..max_iter = %lld", fn, (long long)iteration, (long long)max_iter);
    GAE_REQUIRE(tol >= 0.0 && tol <= DBL_MAX, GAE_E_RANGE, "%s: tol = %g is negative or not finite", fn, tol);
    GAE_REQUIRE(lambdas, GAE_E_NULL, "%s: lambdas is NULL", fn);
    GAE_REQUIRE(coef && intercept && info && n_iter && converged && status, GAE_E_NULL,
                "%s: coef / intercept / info / n_iter / converged / status is NULL", fn);
    GAE_REQUIRE(workspace, GAE_E_NULL, "%s: workspace is NULL", fn);
    GAE_REQUIRE(workspace_bytes >= p.need, GAE_E_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn,
                (long long)workspace_bytes, (long long)p.need);
    const Shape s = shape_of(int(d), int(c));
    gae::Carver cv(workspace);
    UpdateArgs a;
    a.d = int(d); a.c = int(c); a.L = int(n_lambdas); a.lambdas = lambdas;
    a.model_lo = int(model_lo); a.model_count = int(model_count); a.slabs = p.slabs;
    a.iteration = int(iteration); a.max_iter = int(max_iter); a.tol = tol; a.pivot = pivot;
    a.lay = carve(cv, p, s);
    a.coef = coef; a.icpt = intercept; a.info = info; a.n_iter = n_iter; a.converged = converged; a.status = status;
    return gae::launch_lds<&logreg_update_kernel>("logreg_update_kernel", model_count, kThreads, update_lds(s),
                                                  gae::as_stream(stream), a);
}

extern "C" int gae_logreg_predict(const float *X, int64_t ldx, int64_t n, int64_t d, int64_t c, const double *coef,
                                  const double *intercept, const float *pivot, int32_t *labels, float *proba, int64_t ldp,
                                  gae_logreg_status *status, void *stream)
{
    const char *fn = "gae_logreg_predict";
    Plan p;
    if (const int rc = plan(fn, 0, d, c, 1, 1, 1, p)) return rc;
    GAE_REQUIRE(n >= 0, GAE_E_SIZE, "%s: negative n = %lld", fn, (long long)n);
    GAE_REQUIRE(n < (int64_t(1) << 31), GAE_E_SIZE, "%s: n = %lld beyond int32 row ids", fn, (long long)n);
    GAE_REQUIRE(ldx >= d, GAE_E_SIZE, "%s: leading dimension too small (ldx %lld < d)", fn, (long long)ldx);
    GAE_REQUIRE(!proba || ldp >= c, GAE_E_SIZE, "%s: leading dimension too small (ldp %lld < c)", fn, (long long)ldp);
    GAE_REQUIRE(coef && intercept, GAE_E_NULL, "%s: coef / intercept is NULL", fn);
    GAE_REQUIRE(n == 0 || (X && labels), GAE_E_NULL, "%s: X / labels is NULL", fn);
    GAE_REQUIRE(status, GAE_E_NULL, "%s: status is NULL", fn);
    if (n == 0) return GAE_OK;
    const Shape s = shape_of(int(d), int(c));
    const PredictArgs a{X, ldx, int(n), int(d), int(c), coef, intercept, pivot, labels, proba, ldp, status};
    return gae::launch_lds<&logreg_predict_kernel>("logreg_predict_kernel", cdiv(n, kChunk), kThreads, pass_lds(s, 1),
                                                   gae::as_stream(stream), a);
}
