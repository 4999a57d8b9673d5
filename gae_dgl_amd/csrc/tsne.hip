// K29: exact t-SNE of an embedding into the plane, on the device (ops.tsne, ops.tsne_affinities, GAE.map_nodes,
// GAE.map_graphs).  The contract -- definitions, operation orders, the chunk rule -- is the K29 section of
// include/gae_hip_experimental.h; this file restates only what the code needs to be read.
//
// Y fp32 [n, 2] (ldy).  q_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} q_ij,
// g_i = 4 (alpha sum_j P_ij q_ij (y_i - y_j) - (1 / Z) sum_{j != i} q_ij^2 (y_i - y_j)).
//
// One iteration is THREE ordinary launches, none of which waits on another block:
//   repulsion  grid (row panels, column chunks).  A thread holds R rows in registers (a panel is 256 R rows), a block
//              sweeps ONE chunk of gae_tsne_chunk(n) columns, staged through LDS in tiles of at most 1024 columns (clamped
//              loads; every lane reads the same LDS address: a broadcast).  Per (row, chunk) it leaves one partial
//              (fx, fy, z), added in ascending j.  j = i is left out by predicate, and only in the tiles that meet the
//              panel's own rows (a block-uniform choice between two loops that do the same arithmetic).  The hot loop is
//              VALU only: 2 sub, mul, fma, add, v_rcp_f32, add, mul, 2 fma per pair.  Nothing is written per pair.
//   reduce     per row: the chunk partials in the order of common.h's sum_partials (one lane per row for <= 32 chunks, a
//              wave per row beyond), then the attraction over the row's CSR entries of P in ascending entry order and the
//              row's sum of P log(1 + d^2) in fp64; per block: the rows' z in sum_partials' order -> one Z partial.
//   update     every block adds the Z partials (sum_partials again), then gradient, gains, momentum and step per
//              coordinate; per block an fp64 halving tree of |g|^2 and of the rows' KL terms.  The LAST block to finish
//              (an integer ticket) adds the block pieces in a fixed order and writes the status block.
// No float atomics.  Every kernel returns at once when status.done is set.  The grids are functions of n alone.
//
// Affinities (gae_tsne_affinities): one wave per row, lane l holds neighbour l (k <= 64), fp64 throughout; wave sums
// are the xor butterfly 32, 16, ..., 1, so every lane holds the same bits.
#include "common.h"

namespace {

using gae::cdiv;

constexpr int kThreads = 256;
constexpr int kTileCols = 1024;                    // columns of a chunk staged in LDS at a time
constexpr int kMaxK = 64;
constexpr int kGather = 16;                        // CSR entries of a row the reduce launch has in flight
constexpr int kBisect = 100;                       // GAE_TSNE_BISECT_ITERS
constexpr int64_t kMaxWorkspace = int64_t(1) << 33;        // GAE_TSNE_MAX_WORKSPACE
constexpr uint64_t kKeyXor = 0x2545F4914F6CDD1Dull;        // GAE_TSNE_KEY_XOR

// ---- what both sides derive from n alone
inline int64_t chunk_of(int64_t n) { return n <= 8192 ? 256 : n <= 32768 ? 1024 : 8192; }
inline int rows_per_thread(int64_t n) { return n <= 8192 ? 1 : n <= 32768 ? 2 : 4; }

struct Plan {
    int64_t chunk, chunks, panels;
    int R, L, reduce_rows;             // rows per thread; lanes per row and rows per block of the reduce launch
    int64_t reduce_blocks, update_blocks;
    float *part;                       // [chunks][3][n]: fx, fy, z
    float *rowsum, *attr;              // [2][n] each
    double *klrow;                     // [n]
    float *zpart;                      // [reduce_blocks]
    double *gpart, *klpart;            // [update_blocks] each
    int32_t *badpart;                  // [update_blocks]
    int64_t need;
};

// the checks on (n, nnz), the launch shapes and THE workspace layout, carved from `ws` (NULL: counted only)
int plan(const char *fn, int64_t n, int64_t nnz, void *ws, Plan &p)
{
    GAE_REQUIRE(n >= 0 && nnz >= 0, GAE_E_SIZE, "%s: negative size (n = %lld, nnz = %lld)", fn, (long long)n, (long long)nnz);
    GAE_REQUIRE(n < (int64_t(1) << 31) && nnz < (int64_t(1) << 31), GAE_E_SIZE, "%s: n = %lld / nnz = %lld beyond int32",
                fn, (long long)n, (long long)nnz);
    p.chunk = chunk_of(n);
    p.chunks = cdiv(n, p.chunk);
    p.R = rows_per_thread(n);
    p.panels = cdiv(n, int64_t(kThreads) * p.R);
    p.L = p.chunks > 32 ? 64 : 1;
    p.reduce_rows = kThreads / p.L;
    p.reduce_blocks = cdiv(n, p.reduce_rows);
    p.update_blocks = cdiv(n, kThreads);
    GAE_REQUIRE(12.0 * double(n) * double(p.chunks) <= double(kMaxWorkspace), GAE_E_SIZE,
                "%s: n = %lld needs %.0f bytes of partials, above the cap of %lld", fn, (long long)n,
                12.0 * double(n) * double(p.chunks), (long long)kMaxWorkspace);
    gae::Carver c(ws);
    p.part = c.take<float>(3 * n * p.chunks);
    p.rowsum = c.take<float>(2 * n);
    p.attr = c.take<float>(2 * n);
    p.klrow = c.take<double>(n);
    p.zpart = c.take<float>(p.reduce_blocks);
    p.gpart = c.take<double>(p.update_blocks);
    p.klpart = c.take<double>(p.update_blocks);
    p.badpart = c.take<int32_t>(p.update_blocks);
    p.need = c.bytes() > 256 ? c.bytes() : 256;
    return GAE_OK;
}

// ---------------------------------------------------------------------------------------------------- init
__global__ __launch_bounds__(kThreads) void tsne_init_kernel(float *Y, int64_t ldy, int64_t n, uint64_t key)
{
    const int64_t e = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (e >= 2 * n) return;
    uint32_t c[4];
    gae::philox4x32_10(uint64_t(e), 0, key, c);
    const float u = float(c[0] >> 8) * (1.0f / 16777216.0f);           // exact
    Y[(e >> 1) * ldy + (e & 1)] = (2.0f * u - 1.0f) * 1e-4f;             // 2u - 1 exact: one rounding
}

// ---------------------------------------------------------------------------------------------------- affinities
struct AffArgs {
    const int32_t *index;
    const float *dist2;
    int64_t ld, n;
    int k;
    double target;                     // log(perplexity)
    float *p_out;
    int64_t ldp;
    double *perp_out;
};

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(kThreads) void tsne_affinities_kernel(const AffArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = int64_t(blockIdx.x) * (kThreads / 64) + (threadIdx.x >> 6);
    if (row >= a.n) return;                                            // wave-uniform
    const bool in = lane < a.k;
    const int64_t off = row * a.ld + (in ? lane : 0);
    const int idx = a.index[off];
    const float dv = a.dist2[off];
    const bool valid = in && idx >= 0 && dv - dv == 0.f;               // finite distance of a real neighbour
    const int count = __popcll(__ballot(valid));
    double dmin = valid ? double(dv) : INFINITY;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dmin = fmin(dmin, __shfl_xor(dmin, o, 64));
    const double D = valid ? double(dv) - dmin : 0.0;
    double p, perp;
    if (count < 2) {
        p = valid ? 1.0 : 0.0;
        perp = double(count);
    } else {
        double beta = 1.0, lo = 0.0, hi = 0.0;
        bool open = true;                                              // no upper end of the bracket yet
        double e = 0.0, S = 1.0, H = 0.0;
        for (int it = 0; it <= kBisect; ++it) {
            e = valid ? exp(-beta * D) : 0.0;
            S = wave_sum(e);
            const double T = wave_sum(D * e);
            H = log(S) + beta * T / S;
            if (it == kBisect) break;                                  // the last pass only evaluates the final beta
            if (H > a.target) {
                lo = beta;
                beta = open ? beta * 2.0 : 0.5 * (beta + hi);
            } else {
                hi = beta;
                open = false;
                beta = 0.5 * (lo + beta);
            }
        }
        p = e / S;
        perp = exp(H);
    }
    if (in) a.p_out[row * a.ldp + lane] = float(p);
    if (lane == 0) a.perp_out[row] = perp;
}

// ---------------------------------------------------------------------------------------------------- repulsion
struct RepArgs {
    const float *Y;
    int64_t ldy;
    int n, chunk, chunk_lo;
    float *part;
    const gae_tsne_status *status;     // NULL: always runs
};

template <int R, bool MASKED>
__device__ __forceinline__ void sweep_tile(const float2 *ys, int cnt, int t0, const int (&row)[R], const float (&yx)[R],
                                           const float (&yy)[R], float (&fx)[R], float (&fy)[R], float (&z)[R])
{
#pragma unroll 4
    for (int jj = 0; jj < cnt; ++jj) {
        const float2 yj = ys[jj];                                      // the same address in every lane: a broadcast
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float dx = yx[r] - yj.x, dy = yy[r] - yj.y;
            const float d2 = fmaf(dy, dy, dx * dx);
            float q = __builtin_amdgcn_rcpf(1.0f + d2);                // v_rcp_f32
            if (MASKED) q = t0 + jj == row[r] ? 0.f : q;
            z[r] += q;
            const float q2 = q * q;
            fx[r] = fmaf(q2, dx, fx[r]);
            fy[r] = fmaf(q2, dy, fy[r]);
        }
    }
}

template <int R>
__global__ __launch_bounds__(kThreads) void tsne_repulsion_kernel(const RepArgs a)
{
    __shared__ float2 ys[kTileCols];
    if (a.status && a.status->done) return;
    const int n = a.n, tid = threadIdx.x;
    const int c = a.chunk_lo + int(blockIdx.y);
    const int j0 = c * a.chunk;                                        // < n: the host launches existing chunks only
    const int j1 = j0 + a.chunk < n ? j0 + a.chunk : n;
    const int W = a.chunk < kTileCols ? a.chunk : kTileCols;
    const int row0 = int(blockIdx.x) * kThreads * R;
    int row[R];
    float yx[R], yy[R], fx[R], fy[R], z[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        row[r] = row0 + r * kThreads + tid;
        const int64_t rc = row[r] < n ? row[r] : n - 1;                // a row past n is clamped, never stored
        yx[r] = a.Y[rc * a.ldy];
        yy[r] = a.Y[rc * a.ldy + 1];
        fx[r] = fy[r] = z[r] = 0.f;
    }
    for (int t0 = j0; t0 < j1; t0 += W) {
        __syncthreads();                                               // the previous tile is consumed
        for (int e = tid; e < W; e += kThreads) {
            const int64_t jc = t0 + e < n ? t0 + e : n - 1;            // clamped: the loads carry no branch
            ys[e] = make_float2(a.Y[jc * a.ldy], a.Y[jc * a.ldy + 1]);
        }
        __syncthreads();
        const int cnt = j1 - t0 < W ? j1 - t0 : W;                     // columns past n are never added
        if (t0 < row0 + kThreads * R && t0 + W > row0)                 // block-uniform: this tile meets the panel's rows
            sweep_tile<R, true>(ys, cnt, t0, row, yx, yy, fx, fy, z);
        else
            sweep_tile<R, false>(ys, cnt, t0, row, yx, yy, fx, fy, z);
    }
    float *out = a.part + int64_t(c) * 3 * n;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (row[r] < n) {
            out[row[r]] = fx[r];
            out[int64_t(n) + row[r]] = fy[r];
            out[2 * int64_t(n) + row[r]] = z[r];
        }
    }
}

// ---------------------------------------------------------------------------------------------------- reduce
struct RedArgs {
    const float *Y;
    int64_t ldy;
    int n, L;
    int64_t chunks, nnz;
    const float *part;
    const int32_t *indptr, *indices;
    const float *P;
    float *rowsum, *attr;
    double *klrow;
    float *zpart;
    const gae_tsne_status *status;
};

__global__ __launch_bounds__(kThreads) void tsne_reduce_kernel(const RedArgs a)
{
    __shared__ float zs[kThreads];
    if (a.status->done) return;
    const int n = a.n, L = a.L, RB = kThreads / L;
    const int lr = threadIdx.x / L, lane = threadIdx.x % L;
    const int64_t row = int64_t(blockIdx.x) * RB + lr;
    const bool in = row < n;
    const int64_t rc = in ? row : n - 1;
    const int64_t stride = 3 * int64_t(n);
    const float fx = gae::sum_partials(a.part + rc, a.chunks, stride, lane, L);
    const float fy = gae::sum_partials(a.part + n + rc, a.chunks, stride, lane, L);
    const float z = gae::sum_partials(a.part + 2 * int64_t(n) + rc, a.chunks, stride, lane, L);
    if (in && lane == 0) {
        const float yx = a.Y[rc * a.ldy], yy = a.Y[rc * a.ldy + 1];
        int64_t e0 = a.indptr[rc], e1 = a.indptr[rc + 1];
        e1 = e1 < a.nnz ? e1 : a.nnz;                                  // a malformed CSR stays inside its arrays
        e0 = e0 > 0 ? e0 : 0;
        float ax = 0.f, ay = 0.f;
        double kl = 0.0;
        for (int64_t eb = e0; eb < e1; eb += kGather) {                // ascending entries, kGather gathers in flight
            int64_t j[kGather];
            float p[kGather], xj[kGather], yj[kGather];
#pragma unroll
            for (int u = 0; u < kGather; ++u) {
                const int64_t e = eb + u < e1 ? eb + u : e1 - 1;       // clamped: the loads carry no branch
                const unsigned ju = unsigned(a.indices[e]);
                j[u] = ju < unsigned(n) ? ju : unsigned(n - 1);
                p[u] = a.P[e];
            }
#pragma unroll
            for (int u = 0; u < kGather; ++u) {
                xj[u] = a.Y[j[u] * a.ldy];
                yj[u] = a.Y[j[u] * a.ldy + 1];
            }
#pragma unroll
            for (int u = 0; u < kGather; ++u) {
                if (eb + u < e1) {
                    const float dx = yx - xj[u], dy = yy - yj[u];
                    const float d2 = fmaf(dy, dy, dx * dx);
                    const float w = p[u] / (1.0f + d2);                // IEEE division here: not the hot loop
                    ax = fmaf(w, dx, ax);
                    ay = fmaf(w, dy, ay);
                    kl += double(p[u]) * log1p(double(d2));
                }
            }
        }
        a.rowsum[row] = fx;
        a.rowsum[int64_t(n) + row] = fy;
        a.attr[row] = ax;
        a.attr[int64_t(n) + row] = ay;
        a.klrow[row] = kl;
    }
    if (lane == 0) zs[lr] = in ? z : 0.f;
    __syncthreads();
    if (RB > 32) {
        if (threadIdx.x < 64) {                                        // the rows' z as a list of RB partials
            const float s = gae::sum_partials(zs, RB, 1, threadIdx.x, 64);
            if (threadIdx.x == 0) a.zpart[blockIdx.x] = s;
        }
    } else if (threadIdx.x == 0) {
        a.zpart[blockIdx.x] = gae::sum_partials(zs, RB, 1, 0, 1);
    }
}

// ---------------------------------------------------------------------------------------------------- update
struct UpdArgs {
    float *Y;
    int64_t ldy;
    int n;
    int64_t zparts;
    const float *rowsum, *attr;
    const double *klrow;
    const float *zpart;
    double *gpart, *klpart;
    int32_t *badpart;
    float *vel, *gains;
    float alpha, mu, eta;
    double min_grad_norm;
    gae_tsne_status *status;
};

__device__ __forceinline__ int sign_of(float v) { return (v > 0.f) - (v < 0.f); }

__device__ __forceinline__ double coherent_load(const double *p)
{
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long *>(p),
                                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// fp64 halving tree over the block's 256 values (in LDS): slot t += slot t + off for off = 128, 64, ..., 1
__device__ __forceinline__ void block_tree(double *red)
{
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        __syncthreads();
        if (int(threadIdx.x) < off) red[threadIdx.x] += red[threadIdx.x + off];
    }
    __syncthreads();
}

__global__ __launch_bounds__(kThreads) void tsne_update_kernel(const UpdArgs a)
{
    __shared__ double red_g[kThreads], red_k[kThreads];
    __shared__ float s_z;
    __shared__ int s_bad, s_last;
    gae_tsne_status *st = a.status;
    if (st->done) return;
    const int tid = threadIdx.x, n = a.n;
    if (tid == 0) s_bad = 0;
    if (a.zparts > 32) {
        if (tid < 64) {
            const float s = gae::sum_partials(a.zpart, a.zparts, 1, tid, 64);
            if (tid == 0) s_z = s;
        }
    } else if (tid == 0) {
        s_z = gae::sum_partials(a.zpart, a.zparts, 1, 0, 1);
    }
    __syncthreads();
    const float Z = s_z;
    const float inv_z = 1.0f / Z;
    const int64_t row = int64_t(blockIdx.x) * kThreads + tid;
    double g2 = 0.0, kl = 0.0;
    if (row < n) {
        bool bad = false;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float rep = a.rowsum[int64_t(c) * n + row], att = a.attr[int64_t(c) * n + row];
            const float g = 4.0f * fmaf(a.alpha, att, -(rep * inv_z));
            float v = a.vel[row * 2 + c], gn = a.gains[row * 2 + c];
            gn = sign_of(g) != sign_of(v) ? gn + 0.2f : gn * 0.8f;
            gn = fmaxf(gn, 0.01f);
            v = fmaf(a.mu, v, -((a.eta * gn) * g));
            const float y = a.Y[row * a.ldy + c] + v;
            a.gains[row * 2 + c] = gn;
            a.vel[row * 2 + c] = v;
            a.Y[row * a.ldy + c] = y;
            g2 += double(g) * double(g);
            bad = bad || !(y - y == 0.f);
        }
        kl = a.klrow[row];
        if (bad) atomicAdd(&s_bad, 1);                                 // integers: any order
    }
    red_g[tid] = g2;
    red_k[tid] = kl;
    block_tree(red_g);
    block_tree(red_k);
    if (tid == 0) {
        a.gpart[blockIdx.x] = red_g[0];
        a.klpart[blockIdx.x] = red_k[0];
        a.badpart[blockIdx.x] = s_bad;
        __threadfence();                                               // the pieces are out before the ticket
        const unsigned long long ticket = atomicAdd(reinterpret_cast<unsigned long long *>(&st->ticket), 1ull);
        s_last = ticket == (unsigned long long)(gridDim.x) - 1ull;
    }
    __syncthreads();
    if (!s_last) return;
    // ---- the last block to finish: every block's pieces, thread t adds blocks t, t + 256, ... then the tree
    __threadfence();
    double sg = 0.0, sk = 0.0;
    long long sb = 0;
    for (int64_t b = tid; b < int64_t(gridDim.x); b += kThreads) {
        sg += coherent_load(a.gpart + b);
        sk += coherent_load(a.klpart + b);
        sb += __hip_atomic_load(a.badpart + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    red_g[tid] = sg;
    red_k[tid] = sk;
    block_tree(red_g);
    block_tree(red_k);
    if (tid == 0) s_bad = 0;
    __syncthreads();
    if (sb) atomicAdd(&s_bad, int(sb));
    __syncthreads();
    if (tid == 0) {
        st->iteration += 1;
        st->nonfinite += s_bad;
        st->p_log_d = red_k[0];
        st->z = double(Z);
        st->log_z = log(double(Z));
        st->grad2 = red_g[0];
        st->ticket = 0;
        st->done = sqrt(red_g[0]) <= a.min_grad_norm ? 1 : 0;
    }
}

int check_y(const char *fn, const float *Y, int64_t ldy)
{
    GAE_REQUIRE(Y, GAE_E_NULL, "%s: Y is NULL", fn);
    GAE_REQUIRE(ldy >= 2, GAE_E_SIZE, "%s: leading dimension too small (ldy %lld < 2)", fn, (long long)ldy);
    return GAE_OK;
}

int check_ws(const char *fn, const void *workspace, int64_t bytes, const Plan &p)
{
    GAE_REQUIRE(workspace, GAE_E_NULL, "%s: workspace is NULL", fn);
    GAE_REQUIRE(bytes >= p.need, GAE_E_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn, (long long)bytes,
                (long long)p.need);
    return GAE_OK;
}

} // namespace

extern "C" int64_t gae_tsne_chunk(int64_t n)
{
    GAE_REQUIRE(n >= 0, GAE_E_SIZE, "gae_tsne_chunk: negative n = %lld", (long long)n);
    return chunk_of(n);
}

extern "C" int64_t gae_tsne_workspace_bytes(int64_t n, int64_t nnz)
{
    Plan p;
    if (const int rc = plan("gae_tsne_workspace_bytes", n, nnz, nullptr, p)) return rc;
    return p.need;
}

extern "C" int gae_tsne_init(float *Y, int64_t ldy, int64_t n, uint64_t seed, void *stream)
{
    const char *fn = "gae_tsne_init";
    GAE_REQUIRE(n >= 0 && n < (int64_t(1) << 31), GAE_E_SIZE, "%s: n = %lld outside 0..2^31", fn, (long long)n);
    if (const int rc = check_y(fn, Y, ldy)) return rc;
    if (n == 0) return GAE_OK;
    hipLaunchKernelGGL(tsne_init_kernel, dim3(unsigned(cdiv(2 * n, kThreads))), dim3(kThreads), 0, gae::as_stream(stream), Y,
                       ldy, n, seed ^ kKeyXor);
    GAE_CHECK_LAUNCH("tsne_init_kernel");
    return GAE_OK;
}

extern "C" int gae_tsne_affinities(const int32_t *index, const float *dist2, int64_t ld, int64_t n, int64_t k,
                                   double perplexity, float *p_out, int64_t ldp, double *perplexity_out, void *stream)
{
    const char *fn = "gae_tsne_affinities";
    GAE_REQUIRE(n >= 0 && n < (int64_t(1) << 31), GAE_E_SIZE, "%s: n = %lld outside 0..2^31", fn, (long long)n);
    GAE_REQUIRE(k >= 1 && k <= kMaxK, GAE_E_RANGE, "%s: k = %lld outside 1..64", fn, (long long)k);
    GAE_REQUIRE(perplexity >= 1.0 && perplexity < double(k), GAE_E_RANGE, "%s: perplexity = %g outside [1, k = %lld)", fn,
                perplexity, (long long)k);
    GAE_REQUIRE(ld >= k && ldp >= k, GAE_E_SIZE, "%s: leading dimension below k (ld %lld, ldp %lld)", fn, (long long)ld,
                (long long)ldp);
    GAE_REQUIRE(index && dist2 && p_out && perplexity_out, GAE_E_NULL, "%s: index / dist2 / p_out / perplexity_out is NULL",
                fn);
    if (n == 0) return GAE_OK;
    const AffArgs a{index, dist2, ld, n, int(k), log(perplexity), p_out, ldp, perplexity_out};
    hipLaunchKernelGGL(tsne_affinities_kernel, dim3(unsigned(cdiv(n, kThreads / 64))), dim3(kThreads), 0,
                       gae::as_stream(stream), a);
    GAE_CHECK_LAUNCH("tsne_affinities_kernel");
    return GAE_OK;
}

extern "C" int gae_tsne_repulsion(const float *Y, int64_t ldy, int64_t n, int64_t chunk_lo, int64_t chunk_hi,
                                  const gae_tsne_status *status, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "gae_tsne_repulsion";
    Plan p;
    if (const int rc = plan(fn, n, 0, workspace, p)) return rc;
    GAE_REQUIRE(chunk_lo >= 0 && chunk_lo <= chunk_hi && chunk_hi <= p.chunks, GAE_E_RANGE,
                "%s: chunks [%lld, %lld) outside [0, %lld]", fn, (long long)chunk_lo, (long long)chunk_hi,
                (long long)p.chunks);
    if (const int rc = check_y(fn, Y, ldy)) return rc;
    if (const int rc = check_ws(fn, workspace, workspace_bytes, p)) return rc;
    if (n == 0) return GAE_OK;
    hipStream_t st = gae::as_stream(stream);
    for (int64_t c0 = chunk_lo; c0 < chunk_hi; c0 += 32768) {          // grid.y stays below 65536
        const int64_t cn = chunk_hi - c0 < 32768 ? chunk_hi - c0 : 32768;
        const RepArgs a{Y, ldy, int(n), int(p.chunk), int(c0), p.part, status};
        const dim3 grid{unsigned(p.panels), unsigned(cn)};
        if (p.R == 1)
            hipLaunchKernelGGL(tsne_repulsion_kernel<1>, grid, dim3(kThreads), 0, st, a);
        else if (p.R == 2)
            hipLaunchKernelGGL(tsne_repulsion_kernel<2>, grid, dim3(kThreads), 0, st, a);
        else
            hipLaunchKernelGGL(tsne_repulsion_kernel<4>, grid, dim3(kThreads), 0, st, a);
        GAE_CHECK_LAUNCH("tsne_repulsion_kernel");
    }
    return GAE_OK;
}

extern "C" int gae_tsne_update(float *Y, int64_t ldy, int64_t n, const int32_t *indptr, const int32_t *indices,
                               const float *P, int64_t nnz, float *velocity, float *gains, double exaggeration,
                               double momentum, double learning_rate, double min_grad_norm, gae_tsne_status *status,
                               void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "gae_tsne_update";
    Plan p;
    if (const int rc = plan(fn, n, nnz, workspace, p)) return rc;
    GAE_REQUIRE(n >= 2, GAE_E_SIZE, "%s: n = %lld rows (at least 2: Z is a sum over pairs)", fn, (long long)n);
    GAE_REQUIRE(exaggeration > 0.0 && momentum >= 0.0 && momentum < 1.0 && learning_rate > 0.0 &&
                    min_grad_norm == min_grad_norm,
                GAE_E_RANGE, "%s: exaggeration %g / momentum %g / learning_rate %g / min_grad_norm %g out of range", fn,
                exaggeration, momentum, learning_rate, min_grad_norm);
    if (const int rc = check_y(fn, Y, ldy)) return rc;
    GAE_REQUIRE(indptr && velocity && gains && status, GAE_E_NULL, "%s: indptr / velocity / gains / status is NULL", fn);
    GAE_REQUIRE(nnz == 0 || (indices && P), GAE_E_NULL, "%s: indices / P is NULL", fn);
    if (const int rc = check_ws(fn, workspace, workspace_bytes, p)) return rc;
    hipStream_t st = gae::as_stream(stream);
    const RedArgs ra{Y, ldy, int(n), p.L, p.chunks, nnz, p.part, indptr, indices, P, p.rowsum, p.attr, p.klrow, p.zpart,
                     status};
    hipLaunchKernelGGL(tsne_reduce_kernel, dim3(unsigned(p.reduce_blocks)), dim3(kThreads), 0, st, ra);
    GAE_CHECK_LAUNCH("tsne_reduce_kernel");
    const UpdArgs ua{Y, ldy, int(n), p.reduce_blocks, p.rowsum, p.attr, p.klrow, p.zpart, p.gpart, p.klpart, p.badpart,
                     velocity, gains, float(exaggeration), float(momentum), float(learning_rate), min_grad_norm, status};
    hipLaunchKernelGGL(tsne_update_kernel, dim3(unsigned(p.update_blocks)), dim3(kThreads), 0, st, ua);
    GAE_CHECK_LAUNCH("tsne_update_kernel");
    return GAE_OK;
}
