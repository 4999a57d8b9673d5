// Graph-level readout: mean | sum | max of the node embeddings of every member graph of a batch.
//
// The reference describes it (README.md:54: "GAE feature is a concatenation of mean, sum, and max aggregation of the
// hidden vector H in R^{N x 16}, so its dimension is 48" -- the feature behind the ESOL table, README.md:44-51) but
// does not ship the code; with DGL it is dgl.mean_nodes / sum_nodes / max_nodes over the batched graph of
// train_inductive.py:34.  Segment reduction over graph_ptr: HBM-bound, 4 d bytes read per node, 12 d written per
// graph.  One wave per graph: 64 / DP rows in flight per step (DP = d rounded up to a power of two), a fixed
// butterfly across the row slots -> deterministic.  An empty graph gives zeros in all three blocks.
#include "common.h"

namespace {

template <int DP>
__global__ __launch_bounds__(256) void segment_readout_kernel(const float *__restrict__ Z, int64_t ldz, int d,
                                                              const int64_t *__restrict__ graph_ptr, int64_t n_graphs,
                                                              float *__restrict__ out, int64_t ldo)
{
    constexpr int RS = 64 / DP;                  // row slots of a wave
    const int lane = threadIdx.x & 63, c = lane % DP, slot = lane / DP;
    const int64_t g = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (g >= n_graphs) return;
    const int64_t r0 = graph_ptr[g], r1 = graph_ptr[g + 1];
    float s = 0.f, m = -INFINITY;
    if (c < d)
        for (int64_t r = r0 + slot; r < r1; r += RS) {
            const float v = Z[r * ldz + c];
            s += v;
            m = fmaxf(m, v);
        }
#pragma unroll
    for (int off = DP; off < 64; off <<= 1) {    // slot 0 ends up with (slot 0 + slot 1) + (slot 2 + slot 3) ...
        s += __shfl_xor(s, off, 64);
        m = fmaxf(m, __shfl_xor(m, off, 64));
    }
    if (slot == 0 && c < d) {
        const int64_t cnt = r1 - r0;
        float *o = out + g * ldo;
        o[c] = cnt > 0 ? s / float(cnt) : 0.f;   // mean
        o[d + c] = s;                            // sum
        o[2 * d + c] = cnt > 0 ? m : 0.f;        // max
    }
}

// d > 64: one block column of 64 features per blockIdx.y, rows walked by the whole wave
__global__ __launch_bounds__(256) void segment_readout_wide_kernel(const float *__restrict__ Z, int64_t ldz, int d,
                                                                   const int64_t *__restrict__ graph_ptr,
                                                                   int64_t n_graphs, float *__restrict__ out,
                                                                   int64_t ldo)
{
    const int c = blockIdx.y * 64 + (threadIdx.x & 63);
    const int64_t g = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (g >= n_graphs || c >= d) return;
    const int64_t r0 = graph_ptr[g], r1 = graph_ptr[g + 1];
    float s = 0.f, m = -INFINITY;
    for (int64_t r = r0; r < r1; ++r) {
        const float v = Z[r * ldz + c];
        s += v;
        m = fmaxf(m, v);
    }
    const int64_t cnt = r1 - r0;
    float *o = out + g * ldo;
    o[c] = cnt > 0 ? s / float(cnt) : 0.f;
    o[d + c] = s;
    o[2 * d + c] = cnt > 0 ? m : 0.f;
}

// The gradient of the readout: dZ[r][c] = d_sum[c] + d_mean[c] / n + (r == r* ? d_max[c] : 0) for the rows of graph g,
// r* = the LOWEST row whose value equals the column's maximum (the tie rule of K21, embed_bwd.hip).  One wave per graph
// like the forward: 64 / DP row slots walk the rows, each keeps (max, first row attaining it) of its rows, the slots
// meet in a butterfly that prefers the lower row at equal values; then the same lanes write the rows.  d > 64: DP = 64
// and the wave walks the column blocks one after the other.  HBM-bound: Z is read twice (the second time from cache),
// 4 d bytes written per node.  Every row of dZ is written; no atomics.
__global__ __launch_bounds__(256) void segment_readout_bwd_kernel(const float *__restrict__ Z, int64_t ldz, int d, int DP,
                                                                  const int64_t *__restrict__ graph_ptr,
                                                                  int64_t n_graphs, const float *__restrict__ d_out,
                                                                  int64_t ldd, float *__restrict__ dZ, int64_t lddz)
{
    const int RS = 64 / DP;
    const int lane = threadIdx.x & 63, c0 = lane % DP, slot = lane / DP;
    const int64_t g = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (g >= n_graphs) return;
    const int64_t r0 = graph_ptr[g], r1 = graph_ptr[g + 1];
    if (r1 <= r0) return;
    const float cnt = float(r1 - r0);
    const float *go = d_out + g * ldd;
    for (int cb = 0; cb < d; cb += DP) {             // (one trip unless d > 64)
        const int c = cb + c0;
        const bool live = c < d;
        float m = -INFINITY;
        int64_t rs = -1;
        if (live)
            for (int64_t r = r0 + slot; r < r1; r += RS) {
                const float v = Z[r * ldz + c];
                if (rs < 0 || v > m) { m = v; rs = r; }
            }
        for (int off = DP; off < 64; off <<= 1) {
            const float m2 = __shfl_xor(m, off, 64);
            const int64_t rs2 = __shfl_xor(static_cast<long long>(rs), off, 64);
            if (rs2 >= 0 && (rs < 0 || m2 > m || (m2 == m && rs2 < rs))) { m = m2; rs = rs2; }
        }
        if (live) {
            const float base = go[d + c] + go[c] / cnt, gmax = go[2 * d + c];
            for (int64_t r = r0 + slot; r < r1; r += RS) dZ[r * lddz + c] = r == rs ? base + gmax : base;
        }
    }
}

} // namespace

extern "C" int gae_segment_readout(const float *Z, int64_t ldz, int64_t n_nodes, int64_t d, const int64_t *graph_ptr,
                                   int64_t n_graphs, float *out, int64_t ldo, void *stream)
{
    GAE_REQUIRE(n_nodes >= 0 && d >= 0 && n_graphs >= 0, GAE_E_SIZE, "gae_segment_readout: negative size");
    GAE_REQUIRE(ldz >= d && ldo >= 3 * d, GAE_E_SIZE, "gae_segment_readout: leading dimension too small");
    GAE_REQUIRE(d < (int64_t(1) << 20), GAE_E_SIZE, "gae_segment_readout: d too large");
    if (n_graphs == 0 || d == 0) return GAE_OK;
    GAE_REQUIRE(graph_ptr && out && (Z || n_nodes == 0), GAE_E_NULL, "gae_segment_readout: NULL pointer");
    hipStream_t s = gae::as_stream(stream);
    const unsigned gx = unsigned((n_graphs + 3) / 4);
#define GAE_RO(DP) hipLaunchKernelGGL(segment_readout_kernel<DP>, dim3(gx), dim3(256), 0, s, Z, ldz, int(d), graph_ptr, n_graphs, out, ldo)
    if (d <= 1) GAE_RO(1);
    else if (d <= 2) GAE_RO(2);
    else if (d <= 4) GAE_RO(4);
    else if (d <= 8) GAE_RO(8);
    else if (d <= 16) GAE_RO(16);
    else if (d <= 32) GAE_RO(32);
    else if (d <= 64) GAE_RO(64);
    else
        hipLaunchKernelGGL(segment_readout_wide_kernel, dim3(gx, unsigned((d + 63) / 64)), dim3(256), 0, s, Z, ldz, int(d),
                           graph_ptr, n_graphs, out, ldo);
#undef GAE_RO
    GAE_CHECK_LAUNCH("segment_readout_kernel");
    return GAE_OK;
}

extern "C" int gae_segment_readout_bwd(const float *Z, int64_t ldz, int64_t n_nodes, int64_t d, const int64_t *graph_ptr,
                                       int64_t n_graphs, const float *d_out, int64_t ldd, float *dZ, int64_t lddz,
                                       void *stream)
{
    GAE_REQUIRE(n_nodes >= 0 && d >= 0 && n_graphs >= 0, GAE_E_SIZE,
                "gae_segment_readout_bwd: negative n_nodes = %lld, d = %lld or n_graphs = %lld", (long long)n_nodes,
                (long long)d, (long long)n_graphs);
    GAE_REQUIRE(ldz >= d && lddz >= d, GAE_E_SIZE,
                "gae_segment_readout_bwd: leading dimension too small (ldz %lld, lddz %lld < d = %lld)", (long long)ldz,
                (long long)lddz, (long long)d);
    GAE_REQUIRE(ldd >= 3 * d, GAE_E_SIZE, "gae_segment_readout_bwd: leading dimension too small (ldd %lld < 3 d = %lld)",
                (long long)ldd, (long long)(3 * d));
    GAE_REQUIRE(d < (int64_t(1) << 20), GAE_E_SIZE, "gae_segment_readout_bwd: d = %lld too large", (long long)d);
    if (n_graphs == 0 || d == 0 || n_nodes == 0) return GAE_OK;
    GAE_REQUIRE(graph_ptr && Z && d_out && dZ, GAE_E_NULL, "gae_segment_readout_bwd: graph_ptr / Z / d_out / dZ is NULL");
    int DP = 1;
    while (DP < d && DP < 64) DP <<= 1;
    hipLaunchKernelGGL(segment_readout_bwd_kernel, dim3(unsigned((n_graphs + 3) / 4)), dim3(256), 0,
                       gae::as_stream(stream), Z, ldz, int(d), DP, graph_ptr, n_graphs, d_out, ldd, dZ, lddz);
    GAE_CHECK_LAUNCH("segment_readout_bwd_kernel");
    return GAE_OK;
}
