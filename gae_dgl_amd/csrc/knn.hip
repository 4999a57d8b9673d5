// K24: exact k-nearest-neighbour search of one row set against another (ops.knn, GAE.nearest_nodes, GAE.nearest_graphs).
//
// Queries Q fp32 [m, d] (ldq), database X fp32 [n, d] (ldx); 1 <= d <= 256, 1 <= k <= 64, m, n < 2^31.  The contract --
// candidates, keys, reported values, order, padding -- is the comment of gae_knn in include/gae_hip_experimental.h.
//
// Launches (ordinary ones, no float atomics):
//   half    L2 only: h_j = (fmaf chain of x_jf^2, f ascending from 0.f) / 2 for every database row, into the workspace.
//   sweep   one block per (group of NW panels of 32 queries, column split), one wave per panel.  The products are the
//           tile of decoder_pairs.h: the panel is the B operand (in registers for d <= 64), a tile of 32 database rows
//           the A operand, the same DH, chunk order and mma<DH> as K16 -- with Q = X the product has K16's bits.  Unlike
//           K16's Z the database is not cache-resident at the molecule shape (48 MB at n = 249 455, d = 48), so the block
//           stages every (tile, chunk) ONCE in LDS for its NW waves, h beside it: two buffers, the global loads of the
//           next one issued before the products of the current one, one barrier per (tile, chunk).  key = p - h_j (DOT:
//           h = 0, the product itself).  Every lane's 16 keys belong to one query: the lane keeps its top k in an LDS
//           heap with the worst entry at the root (offer_tile of topk_heap.h, K16's), one max and one compare per tile
//           on the fast path.  NaN, -inf and +inf never enter.  The two lane halves of a query merge their sorted lists
//           (merge_halves); with one split that is the query's list, else it goes to the workspace.
//   merge   S > 1: the S sorted lists of each query are merged by rank (merge_kernel of topk_heap.h, K16's): the order
//           is total, so the result does not depend on S.
//   finish  L2 only: per query the direct distance sum_f (q_f - x_jf)^2 of the k chosen rows (fmaf chain, f ascending
//           from 0.f) replaces the key, and the row is re-sorted by (distance ascending, j ascending) with a rank count
//           inside a lane group; padding (j = -1) gets +inf.
//
// LDS of the sweep: NW (2 k + 16) 256 bytes of heaps and tile scratch, 2 . 32 (2 DH + 4) 4 bytes of tile, 256 bytes of
// h.  NW = 4 whenever that fits 160 KB (every shape but d > 32 with k = 64), else 2.  Accumulators in VGPRs
// (-amdgpu-mfma-vgpr-form, _build.py): every one is compared.
#include <float.h>

#include "decoder_pairs.h"
#include "row_search.h"
#include "topk_heap.h"

namespace {

using namespace gae::pairs;
using namespace gae::search;
using namespace gae::topk;
using gae::cdiv;

constexpr int kMaxD = 256;
constexpr int64_t kLdsLimit = 160 * 1024;

struct KnnArgs : SearchArgs {
    const float *Q, *X;
    int d, nch, l2;
    const float *half;                     // [n] (L2)
};

inline int64_t sweep_lds(int nw, int64_t d, int64_t k)
{
    return int64_t(nw) * lists_bytes(int(k)) + 2 * kTile * (2 * dh_of(d) + 4) * 4 + 2 * kTile * 4;
}
inline int waves_of(int64_t d, int64_t k) { return sweep_lds(4, d, k) <= kLdsLimit ? 4 : 2; }

// the workspace: |x|^2 / 2 of the corpus in front of the partial lists, whose bound is for blocks of at most 4 panels
int plan(const char *fn, int64_t m, int64_t n, int64_t d, int64_t k, int splits, void *ws, Plan<float> &p)
{
    return carve(fn, "d", d, kMaxD, m, n, k, splits, kRows * 4, ws, p);
}

// ------------------------------------------------------------------------------------------------------ half
__global__ __launch_bounds__(256) void knn_half_kernel(const float *X, int64_t ldx, int n, int d, float *half)
{
    const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (j >= n) return;
    const float *xp = X + j * ldx;
    float s = 0.f;
    for (int f = 0; f < d; ++f) s = fmaf(xp[f], xp[f], s);
    half[j] = 0.5f * s;
}

// ------------------------------------------------------------------------------------------------------ sweep
template <int DH, bool ONE, int NW>
__global__ __launch_bounds__(64 * NW) void knn_kernel(const KnnArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int W = 2 * DH, pitch = W + 4, T = 64 * NW;
    constexpr int PF = kTile * W / T;                  // staged floats per thread and (tile, chunk)
    static_assert(PF * T == kTile * W, "the tile is a whole number of block passes");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, h = lane >> 5;
    const int k = a.k;
    float *tile = lds;                                 // [2][kTile][pitch]: the A operand's image of a (tile, chunk)
    float *hs = tile + 2 * kTile * pitch;              // [2][kTile]: h of a tile's rows
    float *wl = hs + 2 * kTile + wave * (2 * k + 16) * 64;
    float *ls = wl;                                    // [k][64] keys of each lane's list
    int *lj = reinterpret_cast<int *>(wl + k * 64);    // [k][64] indices
    float *scr = wl + 2 * k * 64;                      // [16][64] keys of a tile that has a passing lane
    const int64_t blockp = blockIdx.x / a.S;
    const int split = blockIdx.x % a.S;
    const int64_t i64 = (blockp * NW + wave) * kRows + col;
    const bool row_ok = i64 < a.m;
    const int i = row_ok ? int(i64) : -1;

    // ---- the block's column part [pb, pe): S parts of whole tiles
    const int64_t L = ((int64_t(a.n) + a.S - 1) / a.S + kTile - 1) / kTile * kTile;
    const int64_t pb = L * split < a.n ? L * split : a.n;
    const int64_t pe = pb + L < a.n ? pb + L : a.n;
    const int ntile = int((pe - pb + kTile - 1) / kTile);
    const int nit = ntile * a.nch;                     // (tile, chunk) steps, chunks inside a tile

    // ---- the panel rows (B operand)
    float zr[DH];
    auto load_row = [&](int q) {
#pragma unroll
        for (int s = 0; s < DH; ++s) {
            const int f = feat0<DH>(q, h) + s;
            zr[s] = (row_ok && f < a.d) ? a.Q[i64 * a.ldq + f] : 0.f;
        }
    };
    if constexpr (ONE) load_row(0);

    // ---- staging: element e = tid + u T of a (tile, chunk) is row e / W, feature e % W of the chunk
    float pf[PF];
    float pfh = 0.f;
    auto fetch = [&](int it) {
        const int t = it / a.nch, q = it - t * a.nch;
        const int64_t c0 = pb + int64_t(t) * kTile;
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int e = tid + u * T, r = e / W, f = q * W + e % W;
            pf[u] = (c0 + r < pe && f < a.d) ? a.X[(c0 + r) * a.ldx + f] : 0.f;
        }
        if (q == 0 && tid < kTile) pfh = (a.l2 && c0 + tid < pe) ? a.half[c0 + tid] : 0.f;
    };
    auto stash = [&](int it) {
        const int t = it / a.nch, q = it - t * a.nch;
        float *dst = tile + (it & 1) * kTile * pitch;
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int e = tid + u * T;
            dst[(e / W) * pitch + e % W] = pf[u];
        }
        if (q == 0 && tid < kTile) hs[(t & 1) * kTile + tid] = pfh;
    };
    if (nit > 0) { fetch(0); stash(0); }
    __syncthreads();

    int cnt = 0;
    float thr = -FLT_MAX;                              // key of the k-th entry once the list is full
    int thr_j = INT32_MAX;
    v16f acc = zero_acc();
    for (int it = 0; it < nit; ++it) {
        const int t = it / a.nch, q = it - t * a.nch;
        if (it + 1 < nit) fetch(it + 1);               // in flight during this step's products
        if constexpr (!ONE) load_row(q);
        float za[DH];
        const float *cp = tile + (it & 1) * kTile * pitch + col * pitch + h * DH;
#pragma unroll
        for (int s = 0; s < DH; ++s) za[s] = cp[s];
        if (q == 0) acc = zero_acc();
        acc = mma<DH>(acc, za, zr);
        if (q == a.nch - 1) {
            const int64_t c0 = pb + int64_t(t) * kTile;
            const float *hp = hs + (t & 1) * kTile;
            float key[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) key[r] = acc[r] - hp[tile_col(0, r, h)];
            // ---- selection (offer_tile, topk_heap.h): past the part, +inf (no candidate) and the same index
            offer_tile(key, row_ok, scr, ls, lj, lane, k, cnt, thr, thr_j, [&](int r, float s) {
                const int64_t jj = tile_col(c0, r, h);
                if (jj >= pe || !(s <= FLT_MAX)) return -1;
                return a.excl_same && int(jj) == i ? -1 : int(jj);
            });
        }
        if (it + 1 < nit) stash(it + 1);               // the buffer step it - 1 read; every wave is past that barrier
        __syncthreads();
    }
    heap_sort(ls, lj, lane, cnt);
    // ---- merge the two lane halves of each query; lane h = 0 writes the list
    __syncthreads();
    const int pcnt = __shfl_down(cnt, 32, 64);
    if (h == 0 && row_ok) {
        const bool direct = a.S == 1;
        float *os = direct ? a.value_out + i64 * a.ldo : a.part_s + (int64_t(split) * a.m + i64) * k;
        int32_t *oj = direct ? a.index_out + i64 * a.ldo : a.part_j + (int64_t(split) * a.m + i64) * k;
        merge_halves(ls, lj, lane, k, cnt, pcnt, [&](int t, float s, int j) { os[t] = s; oj[t] = j; });
    }
}

// ------------------------------------------------------------------------------------------------------ finish
// L2: a group of G = 2^ceil(log2 k) lanes per query; lane e holds entry e of the query's list.
// The row is rewritten IN PLACE: that is safe only because G <= 64 divides the wave, so a group never leaves one wave,
// every lane's load of oj[e] comes before the shuffles and every store after them in the wave's one instruction stream.
// A block size that is no multiple of 64, or loads moved behind the shuffles, would break it.
__global__ __launch_bounds__(256) void knn_finish_kernel(const KnnArgs a, int G)
{
    const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
    const int64_t row = t / G;
    const int e = int(t % G);
    const bool mine = row < a.m && e < a.k;
    float *os = a.value_out + (mine ? row : 0) * a.ldo;
    int32_t *oj = a.index_out + (mine ? row : 0) * a.ldo;
    const int j = mine ? oj[e] : -1;
    float dist = INFINITY;
    if (j >= 0) {
        const float *qp = a.Q + row * a.ldq, *xp = a.X + int64_t(j) * a.ldx;
        dist = 0.f;
        for (int f = 0; f < a.d; ++f) {
            const float df = qp[f] - xp[f];
            dist = fmaf(df, df, dist);
        }
    }
    int rank = 0;
    for (int u = 0; u < G; ++u) {                      // every lane of the wave takes part in the shuffles
        const int ju = __shfl(j, u, G);
        const float du = __shfl(dist, u, G);
        if (ju >= 0 && (du < dist || (du == dist && ju < j))) ++rank;
    }
    if (mine) {
        const int slot = j >= 0 ? rank : e;            // padding stays where it is, behind the valid entries
        os[slot] = dist;
        oj[slot] = j;
    }
}

template <int NW>
int launch_sweep(int64_t blocks, size_t lds, hipStream_t st, const KnnArgs &a)
{
    return dispatch(a.d, [&](auto dh, auto one) {
        return gae::launch_lds<&knn_kernel<dh, one, NW>>("knn_kernel", blocks, 64 * NW, lds, st, a);
    });
}

} // namespace

extern "C" int64_t gae_knn_workspace_bytes(int64_t m, int64_t n, int64_t d, int64_t k, int splits)
{
    Plan<float> p;
    if (const int rc = plan("gae_knn_workspace_bytes", m, n, d, k, splits, nullptr, p)) return rc;
    return p.need;
}

extern "C" int gae_knn(const float *Q, int64_t ldq, int64_t m, const float *X, int64_t ldx, int64_t n, int64_t d, int64_t k,
                       int metric, int flags, int splits, int32_t *index_out, float *value_out, int64_t ldo,
                       void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "gae_knn";
    Plan<float> p;
    if (const int rc = plan(fn, m, n, d, k, splits, workspace, p)) return rc;
    GAE_REQUIRE(metric == GAE_KNN_L2 || metric == GAE_KNN_DOT, GAE_E_RANGE, "%s: unknown metric %d", fn, metric);
    if (const int rc = check_call(fn, "d", d, flags, ldq, ldx, ldo, m, n, k, Q, X, index_out, value_out, workspace,
                                  workspace_bytes, p.need))
        return rc;
    if (m == 0) return GAE_OK;

    const int nw = waves_of(d, k);
    const int S = splits_of(m, n, kRows * nw, splits);
    KnnArgs a;
    fill(a, ldq, ldx, ldo, m, n, k, S, flags, value_out, index_out, p.part);
    a.Q = Q; a.X = X; a.d = int(d);
    a.nch = chunks_of(d);
    a.l2 = metric == GAE_KNN_L2 ? 1 : 0;
    a.half = p.rows;
    hipStream_t st = gae::as_stream(stream);

    // every grid of the call, before the first launch
    int G = 1;
    while (G < k) G *= 2;
    const int64_t blocks = cdiv(m, int64_t(kRows) * nw) * S;
    const int64_t merge_blocks = cdiv(m * S * k, 256), finish_blocks = cdiv(m * G, 256);
    GAE_REQUIRE(blocks < (int64_t(1) << 31) && merge_blocks < (int64_t(1) << 31) && finish_blocks < (int64_t(1) << 31),
                GAE_E_SIZE, "%s: a grid of %lld / %lld / %lld blocks", fn, (long long)blocks, (long long)merge_blocks,
                (long long)finish_blocks);
    if (a.l2 && n > 0) {
        hipLaunchKernelGGL(knn_half_kernel, dim3(unsigned(cdiv(n, 256))), dim3(256), 0, st, X, ldx, int(n), int(d),
                           p.rows);
        GAE_CHECK_LAUNCH("knn_half_kernel");
    }
    const size_t lds = size_t(sweep_lds(nw, d, k));
    if (const int rc = nw == 4 ? launch_sweep<4>(blocks, lds, st, a) : launch_sweep<2>(blocks, lds, st, a)) return rc;
    if (S > 1) {
        const MergeArgs<int32_t> ma{a.part_s, a.part_j, m, a.k, S, value_out, index_out, ldo};
        hipLaunchKernelGGL(merge_kernel<int32_t>, dim3(unsigned(merge_blocks)), dim3(256), 0, st, ma);
        GAE_CHECK_LAUNCH("knn_merge_kernel");
    }
    if (a.l2) {
        hipLaunchKernelGGL(knn_finish_kernel, dim3(unsigned(finish_blocks)), dim3(256), 0, st, a, G);
        GAE_CHECK_LAUNCH("knn_finish_kernel");
    }
    return GAE_OK;
}
