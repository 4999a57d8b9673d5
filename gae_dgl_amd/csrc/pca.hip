// K31: principal components of a frozen feature (ops.pca, ops.pca_transform, GAE.pca_nodes, GAE.pca_graphs).
//
// The contract -- centring, the tournament ordering, every rotation, the order inside a round, the stopping rule, the
// ordering and sign of the output, the projection's chains, the status block -- is the K31 comment of
// include/gae_hip_experimental.h; tests/pca_ref.py restates it in numpy.  This file is compiled without contraction.
//
// Launches (ordinary ones; no float atomics, integer atomics on counters only):
//   solve      ONE block of 512 threads.  The d x d fp64 matrix lives in LDS for the whole launch (129 KB at d = 128), V^T
//              beside it for d <= 96 and in the workspace beyond.  A round: the first m = ceil(d / 2) threads work out the
//              rotations of the round's pairs from the matrix as it stands (barrier); then every thread takes its 2 x 2
//              blocks (k <= l of the m (m + 1) / 2 pair blocks: it reads a block's four values, applies the column and
//              the row rotation in registers and writes the block and its transpose -- blocks are disjoint, so the
//              update is in place) and its (pair, column) items of V^T (barrier).  The blocks a thread owns are the
//              same in every round and are decoded once.  Two barriers per round, (d - 1) rounds per sweep.
//   transform  blocks of four waves walk tiles of 64 listed rows: the tile is staged in LDS as x - m (one fp32
//              subtraction, coalesced reads, zero past d and past the list), each wave multiplies its 16 rows by V^T (fp32
//              in LDS, zero padded to tiles of 16 components) on v_mfma_f32_16x16x4_f32: lane l feeds A[l & 15][l >> 4] and
//              B[l >> 4][l & 15]; the result has column l & 15 and rows 4 (l >> 4) + reg.  Waves split rows, never j.
//
// LDS: solve 8 d (d | 1) (twice for d <= 96; the odd pitch keeps a column walk off a single bank) + 56 m + 32 d + 64 bytes; transform 4 (dP kP + 64 (dP + 4) + dP + 2 kP + 64).
#include "common.h"
#include "cholesky.h"
#include "fold_lists.h"

namespace {

using gae::cdiv;
using gae::finite32;
using gae::up256;
using gae::upper_at;
using gae::v4f;

constexpr int kMaxD = GAE_PCA_MAX_D, kMaxT = 8;
constexpr int kSolveThreads = 512;
constexpr int kMaxM = kMaxD / 2;
constexpr int kMaxBlocks = (kMaxM * (kMaxM + 1) / 2 + kSolveThreads - 1) / kSolveThreads;      // 2 x 2 blocks per thread
constexpr int kVInLds = 96;                // V^T shares LDS with the matrix up to this d (2 . 96 . 97 . 8 = 146 KB)
constexpr int kVBatch = 4;                 // V^T items a thread loads before it stores
constexpr double kTol = 0x1p-53;

// ------------------------------------------------------------------------------------------------------ solve
struct SolveArgs {
    const double *stats;
    int d, t, W, k;
    const float *pivot;
    double *mean, *values, *comps;
    gae_pca_status *st;
    double *Vg;                            // [d][d | 1] in the workspace (d > kVInLds)
};

inline size_t solve_lds(int64_t d)
{
    const int64_t m = (d + 1) / 2;
    return size_t((d * (d | 1)) * (d <= kVInLds ? 2 : 1) + 4 * m + 4 * d) * 8 + size_t(2 * m + d) * 4 + 64;
}

__global__ __launch_bounds__(kSolveThreads) void pca_solve_kernel(const SolveArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int d = a.d, W = a.W, k = a.k, tid = threadIdx.x;
    const int m = (d + 1) / 2, dp = 2 * m, nb = m * (m + 1) / 2;
    const int ld = d | 1;                              // an odd pitch: a column walk touches every LDS bank
    double *A = lds;                                   // [d][ld]
    double *Vl = A + d * ld;                           // [d][ld] when d <= kVInLds
    double *Vt = d <= kVInLds ? Vl : a.Vg;             // row i = column i of V
    double *rc = Vl + (d <= kVInLds ? d * ld : 0);      // [m] cosines
    double *rs = rc + m;                               // [m] sines
    double *rt = rs + m;                               // [m] tangents
    double *ro = rt + m;                               // [m] a_pq at the start of the round
    double *mu = ro + m;                               // [d]; later the eigenvalues
    double *s0 = mu + d;                               // [d]; later the row sums of the off-diagonal norm
    double *sg = s0 + d;                               // [d] signs of the components
    double *spare = sg + d;                            // [d]
    int *pp = reinterpret_cast<int *>(spare + d);      // [m] smaller index of a pair
    int *qq = pp + m;                                  // [m] larger index; >= d: the pair sits out
    int *order = qq + m;                               // [d]
    int *cnt = order + d;                              // [1] rotations so far
    const double nan = __builtin_nan("");

    const double c = a.stats[0];
    if (!(c >= 2.0)) {
        for (int j = tid; j < d; j += kSolveThreads) a.mean[j] = nan;
        for (int e = tid; e < k * d; e += kSolveThreads) a.comps[e] = nan;
        for (int e = tid; e < k; e += kSolveThreads) a.values[e] = nan;
        if (tid == 0) {
            a.st->info = -1; a.st->n_sweeps = 0; a.st->n_rotations = 0;
            a.st->off_norm = nan; a.st->total_variance = nan;
        }
        return;
    }
    const double cm1 = c - 1.0;
    for (int j = tid; j < d; j += kSolveThreads) {
        const double s = a.stats[upper_at(0, 1 + j, W)];
        s0[j] = s;
        mu[j] = s / c;
        a.mean[j] = (a.pivot ? double(a.pivot[j]) : 0.0) + mu[j];
    }
    if (tid == 0) *cnt = 0;
    __syncthreads();
    for (int e = tid; e < d * d; e += kSolveThreads) {
        const int i = e / d, j = e % d, lo = i < j ? i : j, hi = i < j ? j : i;
        const double prod = s0[hi] * mu[lo];
        A[i * ld + j] = (a.stats[upper_at(1 + lo, 1 + hi, W)] - prod) / cm1;
        Vt[i * ld + j] = i == j ? 1.0 : 0.0;
    }
    // the thread's blocks, the same in every round: b = l (l + 1) / 2 + k2, k2 <= l
    int bk[kMaxBlocks], bl[kMaxBlocks];
#pragma unroll
    for (int u = 0; u < kMaxBlocks; ++u) {
        const int b = tid + u * kSolveThreads;
        int l = 0;
        if (b < nb) {
            l = int((sqrtf(8.f * float(b) + 1.f) - 1.f) * 0.5f);
            while (l * (l + 1) / 2 > b) --l;
            while ((l + 1) * (l + 2) / 2 <= b) ++l;
        }
        bl[u] = l;
        bk[u] = b < nb ? b - l * (l + 1) / 2 : 0;
    }
    __syncthreads();

    int sweeps = 0, done = 0, info = 1;
    for (int sweep = 0; sweep < GAE_PCA_MAX_SWEEPS; ++sweep) {
        for (int r = 0; r < dp - 1; ++r) {
            if (tid < m) {
                int x, y;
                if (tid == 0) { x = r; y = dp - 1; }
                else { x = (r + tid) % (dp - 1); y = (r - tid + dp - 1) % (dp - 1); }
                const int p = x < y ? x : y, q = x < y ? y : x;
                double cc = 1.0, ss = 0.0, tt = 0.0, apq = 0.0;
                if (q < d) {
                    const double app = A[p * ld + p], aqq = A[q * ld + q];
                    apq = A[p * ld + q];
                    const double bound = kTol * sqrt(fabs(app) * fabs(aqq));
                    if (apq != 0.0 && fabs(apq) > bound) {
                        const double tau = (aqq - app) / (2.0 * apq);
                        const double root = sqrt(1.0 + tau * tau);
                        const double den = fabs(tau) + root;
                        tt = (tau >= 0.0 ? 1.0 : -1.0) / den;
                        cc = 1.0 / sqrt(1.0 + tt * tt);
                        ss = tt * cc;
                        atomicAdd(cnt, 1);
                    } else {
                        apq = 0.0;                                     // a skipped pair: its own block is left as it is
                    }
                }
                pp[tid] = p; qq[tid] = q;
                rc[tid] = cc; rs[tid] = ss; rt[tid] = tt; ro[tid] = apq;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < kMaxBlocks; ++u) {
                if (tid + u * kSolveThreads >= nb) break;
                const int k1 = bk[u], k2 = bl[u];
                const int p = pp[k1], q = qq[k1];
                if (k1 == k2) {
                    const double tt = rt[k1], apq = ro[k1];
                    if (q < d && apq != 0.0) {
                        const double delta = tt * apq;
                        A[p * ld + p] = A[p * ld + p] - delta;
                        A[q * ld + q] = A[q * ld + q] + delta;
                        A[p * ld + q] = 0.0;
                        A[q * ld + p] = 0.0;
                    }
                    continue;
                }
                const int r2 = pp[k2], u2 = qq[k2];                    // k1 < k2: pair k2 is never the one sitting out
                const double c1 = rc[k1], s1 = rs[k1], c2 = rc[k2], s2 = rs[k2];
                if (s1 == 0.0 && s2 == 0.0) continue;                  // both skipped: the identity
                const bool two = q < d;
                const double va = A[p * ld + r2], vb = A[p * ld + u2];
                const double ve = two ? A[q * ld + r2] : 0.0, vf = two ? A[q * ld + u2] : 0.0;
                const double a1 = c2 * va - s2 * vb, b1 = s2 * va + c2 * vb;         // columns (r2, u2)
                const double e1 = c2 * ve - s2 * vf, f1 = s2 * ve + c2 * vf;
                const double a2 = c1 * a1 - s1 * e1, e2 = s1 * a1 + c1 * e1;         // rows (p, q)
                const double b2 = c1 * b1 - s1 * f1, f2 = s1 * b1 + c1 * f1;
                A[p * ld + r2] = a2; A[r2 * ld + p] = a2;
                A[p * ld + u2] = b2; A[u2 * ld + p] = b2;
                if (two) {
                    A[q * ld + r2] = e2; A[r2 * ld + q] = e2;
                    A[q * ld + u2] = f2; A[u2 * ld + q] = f2;
                }
            }
            // V^T rows p, q of every rotated pair; kVBatch items are loaded before the first is stored (the rows of
            // distinct pairs are disjoint), so the loads of a batch overlap when V^T lives in global memory
            for (int e0 = tid; e0 < m * d; e0 += kVBatch * kSolveThreads) {
                double x[kVBatch], y[kVBatch];
                int ip[kVBatch], iq[kVBatch], kk[kVBatch];
#pragma unroll
                for (int u = 0; u < kVBatch; ++u) {
                    const int e = e0 + u * kSolveThreads;
                    kk[u] = -1;
                    if (e < m * d) {
                        const int k1 = e / d, i = e - k1 * d;
                        if (rs[k1] != 0.0) {
                            kk[u] = k1;
                            ip[u] = pp[k1] * ld + i; iq[u] = qq[k1] * ld + i;
                            x[u] = Vt[ip[u]]; y[u] = Vt[iq[u]];
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < kVBatch; ++u) {
                    if (kk[u] < 0) continue;
                    const double c1 = rc[kk[u]], s1 = rs[kk[u]];
                    Vt[ip[u]] = c1 * x[u] - s1 * y[u];
                    Vt[iq[u]] = s1 * x[u] + c1 * y[u];
                }
            }
            __syncthreads();
        }
        ++sweeps;
        const int now = *cnt;
        __syncthreads();                                               // every thread has read the count
        if (now == done) { info = 0; break; }
        done = now;
    }

    // ---- the spectrum: the diagonal, descending, equal values to the lower index
    double *lam = mu, *rowsum = s0;
    for (int i = tid; i < d; i += kSolveThreads) {
        lam[i] = A[i * ld + i];
        double s = 0.0;
        for (int j = 0; j < d; ++j) {
            if (j == i) continue;
            const double v = A[i * ld + j];
            const double sq = v * v;
            s = s + sq;
        }
        rowsum[i] = s;
    }
    __syncthreads();
    for (int i = tid; i < d; i += kSolveThreads) {
        const double v = lam[i];
        int rank = 0;
        for (int j = 0; j < d; ++j) {
            const double w = lam[j];
            // a total order (a NaN, which only non-finite moments give, sorts last): the ranks are a permutation
            const bool before = w > v || (v != v && w == w);
            const bool same = w == v || (w != w && v != v);
            rank += (before || (same && j < i)) ? 1 : 0;
        }
        order[rank] = i;
    }
    __syncthreads();
    for (int cidx = tid; cidx < k; cidx += kSolveThreads) {
        const double *row = Vt + order[cidx] * ld;
        double best = -1.0, at = 0.0;
        for (int i = 0; i < d; ++i) {
            const double v = row[i];
            if (fabs(v) > best) { best = fabs(v); at = v; }
        }
        sg[cidx] = at < 0.0 ? -1.0 : 1.0;
    }
    __syncthreads();
    const bool ok = info == 0;
    if (!ok)
        for (int j = tid; j < d; j += kSolveThreads) a.mean[j] = nan;
    for (int e = tid; e < k * d; e += kSolveThreads) {
        const int cidx = e / d, i = e % d;
        a.comps[e] = ok ? sg[cidx] * Vt[order[cidx] * ld + i] : nan;
    }
    for (int e = tid; e < k; e += kSolveThreads) a.values[e] = ok ? lam[order[e]] : nan;
    if (tid == 0) {
        double off = 0.0, total = 0.0;
        for (int i = 0; i < d; ++i) off = off + rowsum[i];
        for (int i = 0; i < d; ++i) total = total + lam[order[i]];
        a.st->info = info;
        a.st->n_sweeps = sweeps;
        a.st->n_rotations = done;
        a.st->off_norm = ok ? sqrt(off) : nan;
        a.st->total_variance = ok ? total : nan;
    }
}

// ------------------------------------------------------------------------------------------------------ transform
constexpr int kThreads = 256, kWaves = kThreads / gae::kWave;
constexpr int kTileRows = 16 * kWaves;     // listed rows per block pass
constexpr int kMaxKT = kMaxD / 16;
constexpr int kMaxGrid = 1024;

struct ProjArgs {
    const float *X;
    int64_t ldx, ldz;
    int n, d, n_rows, k, whiten;
    const int32_t *rows;
    const double *mean, *comps, *values;
    float *Z;
    gae_pca_status *st;
};

inline int proj_dP(int64_t d) { return int(cdiv(d, 4) * 4); }
inline int proj_kP(int64_t k) { return int(cdiv(k, 16) * 16); }
inline size_t proj_lds(int64_t d, int64_t k)
{
    const int64_t dP = proj_dP(d), kP = proj_kP(k);
    return size_t(dP * kP + kTileRows * (dP + 4) + dP + 2 * kP + kTileRows) * 4;
}

__global__ __launch_bounds__(kThreads) void pca_transform_kernel(const ProjArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float ldsf[];
    const int d = a.d, k = a.k, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int dP = (d + 3) / 4 * 4, kP = (k + 15) / 16 * 16, KT = kP / 16, pitch = dP + 4;
    float *Vs = ldsf;                                  // [dP][kP]: v_cj at j kP + c
    float *Xs = Vs + dP * kP;                          // [kTileRows][pitch]: x - m
    float *ms = Xs + kTileRows * pitch;                // [dP]
    float *scale = ms + dP;                            // [kP]
    int *pos = reinterpret_cast<int *>(scale + kP);    // [kP]: the component's value is > 0
    int *rowbad = pos + kP;                            // [kTileRows]: 1 a non-finite value, 2 a row id outside [0, n)

    for (int e = tid; e < dP * kP; e += kThreads) {
        const int j = e / kP, cidx = e % kP;
        Vs[e] = (j < d && cidx < k) ? float(a.comps[int64_t(cidx) * d + j]) : 0.f;
    }
    for (int j = tid; j < dP; j += kThreads) ms[j] = j < d ? float(a.mean[j]) : 0.f;
    for (int cidx = tid; cidx < kP; cidx += kThreads) {
        float sc = 1.f;
        int on = 1;
        if (a.whiten && cidx < k) {
            const double v = a.values[cidx];
            on = v > 0.0 ? 1 : 0;
            if (on) {
                const double root = sqrt(v);
                sc = float(1.0 / root);
            } else if (blockIdx.x == 0) {
                gae::add_count(&a.st->nonpositive_components, 1);
            }
        }
        scale[cidx] = sc;
        pos[cidx] = on;
    }
    if (tid < kTileRows) rowbad[tid] = 0;
    __syncthreads();

    const int64_t tiles = (int64_t(a.n_rows) + kTileRows - 1) / kTileRows;
    const gae::FoldList list{a.rows, nullptr, 1, a.n_rows};
    const int lr = lane & 15, lq = lane >> 4;
    const int Q = dP / 4, r0 = tid / Q, jq0 = tid % Q, dr = kThreads / Q, djq = kThreads % Q;
    const bool vec = (a.ldx & 3) == 0 && (reinterpret_cast<uintptr_t>(a.X) & 15u) == 0;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t base = tile * kTileRows;
        // four columns per thread and step, (row, column group) advanced without a division; one 16-byte load where the
        // row is aligned and the group lies inside d
        for (int r = r0, jq = jq0; r < kTileRows; r += dr, jq += djq) {
            if (jq >= Q) { jq -= Q; ++r; if (r >= kTileRows) break; }
            const int j = 4 * jq;
            float x[4] = {0.f, 0.f, 0.f, 0.f};
            int live = 0;
            if (base + r < a.n_rows) {
                bool bad_id = false;
                const int id = gae::row_id(list, base + r, a.n, bad_id);
                if (!bad_id) {
                    const float *src = a.X + int64_t(id) * a.ldx + j;
                    live = d - j < 4 ? d - j : 4;
                    if (vec && live == 4) {
                        const float4 v = *reinterpret_cast<const float4 *>(src);
                        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
                    } else {
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (u < live) x[u] = src[u];
                    }
                } else if (jq == 0) {
                    atomicOr(&rowbad[r], 2);
                }
            }
            float4 o;
            bool bad = false;
            float *ov = &o.x;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                bad = bad || (u < live && !finite32(x[u]));
                ov[u] = u < live ? x[u] - ms[j + u] : 0.f;
            }
            if (bad) atomicOr(&rowbad[r], 1);
            *reinterpret_cast<float4 *>(Xs + r * pitch + j) = o;
        }
        __syncthreads();
        if (tid < kTileRows && rowbad[tid]) {
            if (rowbad[tid] & 1) gae::add_count(&a.st->nonfinite_rows, 1);
            if (rowbad[tid] & 2) gae::or_bits(&a.st->errors, GAE_PCA_ERR_ROW_ID);
        }
        v4f acc[kMaxKT];
#pragma unroll
        for (int tt = 0; tt < kMaxKT; ++tt) acc[tt] = v4f{0.f, 0.f, 0.f, 0.f};
        const float *pa = Xs + (16 * wave + lr) * pitch + lq;
        const float *pb = Vs + lq * kP + lr;
        for (int s = 0; s < dP / 4; ++s) {
            const float av = pa[4 * s];
#pragma unroll
            for (int tt = 0; tt < kMaxKT; ++tt)
                if (tt < KT) acc[tt] = gae::mfma4(av, pb[4 * s * kP + 16 * tt], acc[tt]);
        }
#pragma unroll
        for (int tt = 0; tt < kMaxKT; ++tt) {
            if (tt >= KT) break;
            const int cidx = 16 * tt + lr;
            if (cidx >= k) continue;
            const float sc = scale[cidx];
            const int on = pos[cidx];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int r = 16 * wave + 4 * lq + reg;
                if (base + r >= a.n_rows) continue;
                float z = acc[tt][reg];
                if (a.whiten) z = on ? z * sc : 0.f;
                if (rowbad[r]) z = __builtin_nanf("");
                a.Z[(base + r) * a.ldz + cidx] = z;
            }
        }
        __syncthreads();
        if (tid < kTileRows) rowbad[tid] = 0;
        // (the next pass writes rowbad only after its staging loop starts; the barrier after that loop orders the reads)
        __syncthreads();
    }
}

int check_d(const char *fn, int64_t d)
{
    GAE_REQUIRE(d >= 1 && d <= kMaxD, GAE_E_RANGE, "%s: d = %lld outside 1..128", fn, (long long)d);
    return GAE_OK;
}

} // namespace

extern "C" int64_t gae_pca_workspace_bytes(int64_t d)
{
    if (const int rc = check_d("gae_pca_workspace_bytes", d)) return rc;
    return up256(d * (d | 1) * 8) + 256;
}

extern "C" int gae_pca_solve(const double *stats, int64_t d, int64_t t, const float *pivot, int64_t n_rows_used,
                             int64_t n_components, int flags, double *mean, double *values, double *components,
                             gae_pca_status *status, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "gae_pca_solve";
    if (const int rc = check_d(fn, d)) return rc;
    GAE_REQUIRE(t >= 0 && t <= kMaxT, GAE_E_RANGE, "%s: t = %lld outside 0..8", fn, (long long)t);
    GAE_REQUIRE(n_components >= 1 && n_components <= d, GAE_E_RANGE, "%s: n_components = %lld outside 1..d = %lld", fn,
                (long long)n_components, (long long)d);
    GAE_REQUIRE(flags == 0, GAE_E_RANGE, "%s: unknown flags 0x%x", fn, flags);
    GAE_REQUIRE(n_rows_used >= 0 && n_rows_used < (int64_t(1) << 31), GAE_E_SIZE, "%s: n_rows_used = %lld outside 0..2^31 - 1",
                fn, (long long)n_rows_used);
    GAE_REQUIRE(stats, GAE_E_NULL, "%s: stats is NULL", fn);
    GAE_REQUIRE(mean && values && components && status, GAE_E_NULL, "%s: mean / values / components / status is NULL", fn);
    GAE_REQUIRE(workspace, GAE_E_NULL, "%s: workspace is NULL", fn);
    const int64_t need = gae_pca_workspace_bytes(d);
    GAE_REQUIRE(workspace_bytes >= need, GAE_E_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn,
                (long long)workspace_bytes, (long long)need);
    const SolveArgs a{stats, int(d), int(t), int(1 + d + t), int(n_components), pivot, mean, values, components, status,
                      static_cast<double *>(workspace)};
    return gae::launch_lds<&pca_solve_kernel>("pca_solve_kernel", 1, kSolveThreads, solve_lds(d), gae::as_stream(stream), a);
}

extern "C" int gae_pca_transform(const float *X, int64_t ldx, int64_t n, int64_t d, const int32_t *rows, int64_t n_rows,
                                 const double *mean, const double *components, const double *values, int64_t k, int flags,
                                 float *Z, int64_t ldz, gae_pca_status *status, void *stream)
{
    const char *fn = "gae_pca_transform";
    if (const int rc = check_d(fn, d)) return rc;
    GAE_REQUIRE(k >= 1 && k <= d, GAE_E_RANGE, "%s: k = %lld outside 1..d = %lld", fn, (long long)k, (long long)d);
    GAE_REQUIRE((flags & ~GAE_PCA_WHITEN) == 0, GAE_E_RANGE, "%s: unknown flags 0x%x", fn, flags);
    GAE_REQUIRE(n >= 0 && n_rows >= 0, GAE_E_SIZE, "%s: negative n = %lld or n_rows = %lld", fn, (long long)n, (long long)n_rows);
    GAE_REQUIRE(n < (int64_t(1) << 31) && n_rows < (int64_t(1) << 31), GAE_E_SIZE, "%s: n = %lld or n_rows = %lld beyond int32 row ids",
                fn, (long long)n, (long long)n_rows);
    GAE_REQUIRE(ldx >= d && ldz >= k, GAE_E_SIZE, "%s: leading dimension too small (ldx %lld < d or ldz %lld < k)", fn,
                (long long)ldx, (long long)ldz);
    GAE_REQUIRE(rows || n_rows == n, GAE_E_SIZE, "%s: rows is NULL (rows 0 .. n - 1) with n_rows = %lld, n = %lld", fn,
                (long long)n_rows, (long long)n);
    GAE_REQUIRE(n_rows == 0 || (X && Z), GAE_E_NULL, "%s: X / Z is NULL", fn);
    GAE_REQUIRE(mean && components && status, GAE_E_NULL, "%s: mean / components / status is NULL", fn);
    GAE_REQUIRE(!(flags & GAE_PCA_WHITEN) || values, GAE_E_NULL, "%s: GAE_PCA_WHITEN without values", fn);
    if (n_rows == 0) return GAE_OK;
    const ProjArgs a{X, ldx, ldz, int(n), int(d), int(n_rows), int(k), (flags & GAE_PCA_WHITEN) ? 1 : 0, rows, mean, components,
                     values, Z, status};
    const int64_t tiles = cdiv(n_rows, kTileRows);
    return gae::launch_lds<&pca_transform_kernel>("pca_transform_kernel", tiles < kMaxGrid ? tiles : kMaxGrid, kThreads,
                                                  proj_lds(d, k), gae::as_stream(stream), a);
}
