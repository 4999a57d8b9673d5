// K34: exact Tanimoto k-nearest-neighbour search over bit fingerprints (ops.tanimoto_knn).
//
// Queries Q int32 [m, W] (ldq), database X int32 [n, W] (ldx): rows of W 32-bit words; 1 <= W <= 64, 1 <= k <= 64,
// m, n < 2^31.  The contract -- values, order, padding -- is the comment of gae_tanimoto_knn in
// include/gae_hip_experimental.h.
//
// Launches (ordinary ones, no float atomics):
//   count   b_j = popcount of database row j, into the workspace
//   sweep   one block per (256 queries, column split): four waves, ONE QUERY PER LANE, its words in registers (WR = W
//           rounded up to a power of two, zero words beyond W).  A tile of 16 database rows is staged once per block in
//           LDS, b beside it: two buffers, the global loads of the next tile issued before the counts of the current
//           one, one barrier per tile.  Every lane reads the tile at the SAME address (a broadcast: no bank conflict);
//           per word pair one AND and one accumulating bit count on the VALU.  u = a + b - c, key = float(c) / float(u)
//           by the compiler's correctly rounded division (0.f for u = 0): for u <= 4096 different fractions never share
//           a quotient and the quotients keep the exact order, so selecting on the key is selecting on the fraction,
//           and the key is the reported value.  The lane's 16 keys go to offer_tile of topk_heap.h (K16's and K24's
//           tail: the heap in LDS, the running threshold); the sorted list is written by merge_halves with an empty
//           second half.  With one split that is the query's row, else it goes to the workspace.
//   merge   S > 1: merge_kernel of topk_heap.h by rank; the order is total, so the result does not depend on S.
//
// LDS of the sweep: 4 (2 k + 16) 256 bytes of heaps and tile scratch, 2 . 16 . WR . 4 bytes of tile, 128 bytes of b:
// 152 KB at k = 64, W = 64.
#include <float.h>

#include "row_search.h"
#include "topk_heap.h"

namespace {

using namespace gae::search;
using namespace gae::topk;
using gae::cdiv;

constexpr int kMaxW = 64;
constexpr int kTile = 16;                  // database rows per tile: the 16 keys of offer_tile
constexpr int kNW = 4;                     // waves per block
constexpr int kQueries = 64 * kNW;         // queries per block

struct TaniArgs : SearchArgs {
    const int32_t *Q, *X;
    int W;
    const int32_t *bcount;                 // [n]
};

inline int wr_of(int64_t W)
{
    int wr = 1;
    while (wr < W) wr *= 2;
    return wr;
}

inline int64_t sweep_lds(int64_t W, int64_t k)
{
    return int64_t(kNW) * lists_bytes(int(k)) + 2 * kTile * wr_of(W) * 4 + 2 * kTile * 4;
}

// the workspace: the bit counts of the database rows in front of the partial lists
int plan(const char *fn, int64_t m, int64_t n, int64_t W, int64_t k, int splits, void *ws, Plan<int32_t> &p)
{
    return carve(fn, "n_words", W, kMaxW, m, n, k, splits, kQueries, ws, p);
}

// ------------------------------------------------------------------------------------------------------ count
__global__ __launch_bounds__(256) void tanimoto_count_kernel(const int32_t *X, int64_t ldx, int n, int W, int32_t *bcount)
{
    const int64_t j = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (j >= n) return;
    const int32_t *xp = X + j * ldx;
    int b = 0;
    for (int w = 0; w < W; ++w) b += __popc(unsigned(xp[w]));
    bcount[j] = b;
}

// ------------------------------------------------------------------------------------------------------ sweep
template <int WR>
__global__ __launch_bounds__(kQueries) void tanimoto_kernel(const TaniArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int T = kQueries;
    constexpr int PF = (kTile * WR + T - 1) / T;       // staged words per thread and tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = a.k;
    unsigned *tile = reinterpret_cast<unsigned *>(lds);            // [2][kTile][WR]
    int *bs = reinterpret_cast<int *>(tile + 2 * kTile * WR);      // [2][kTile]: b of a tile's rows
    float *wl = reinterpret_cast<float *>(bs + 2 * kTile) + wave * (2 * k + 16) * 64;
    float *ls = wl;                                    // [k][64] keys of each lane's list
    int *lj = reinterpret_cast<int *>(wl + k * 64);    // [k][64] indices
    float *scr = wl + 2 * k * 64;                      // [16][64] keys of a tile that has a passing lane
    const int64_t blockp = blockIdx.x / a.S;
    const int split = blockIdx.x % a.S;
    const int64_t i64 = blockp * kQueries + tid;
    const bool row_ok = i64 < a.m;
    const int i = row_ok ? int(i64) : -1;

    // ---- the block's column part [pb, pe): S parts of whole tiles
    const int64_t L = ((int64_t(a.n) + a.S - 1) / a.S + kTile - 1) / kTile * kTile;
    const int64_t pb = L * split < a.n ? L * split : a.n;
    const int64_t pe = pb + L < a.n ? pb + L : a.n;
    const int ntile = int((pe - pb + kTile - 1) / kTile);

    // ---- the lane's query: its words (zero beyond W) and their count
    unsigned q[WR];
    int qa = 0;
#pragma unroll
    for (int w = 0; w < WR; ++w) {
        q[w] = (row_ok && w < a.W) ? unsigned(a.Q[i64 * a.ldq + w]) : 0u;
        qa += __popc(q[w]);
    }

    // ---- staging: word e = tid + u T of a tile is row e / WR, word e % WR
    unsigned pf[PF];
    int pfb = 0;
    auto fetch = [&](int t) {
        const int64_t c0 = pb + int64_t(t) * kTile;
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int e = tid + u * T, r = e / WR, w = e % WR;
            pf[u] = (e < kTile * WR && c0 + r < pe && w < a.W) ? unsigned(a.X[(c0 + r) * a.ldx + w]) : 0u;
        }
        if (tid < kTile) pfb = c0 + tid < pe ? a.bcount[c0 + tid] : 0;
    };
    auto stash = [&](int t) {
        unsigned *dst = tile + (t & 1) * kTile * WR;
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int e = tid + u * T;
            if (e < kTile * WR) dst[e] = pf[u];
        }
        if (tid < kTile) bs[(t & 1) * kTile + tid] = pfb;
    };
    if (ntile > 0) { fetch(0); stash(0); }
    __syncthreads();

    int cnt = 0;
    float thr = -FLT_MAX;                              // key of the k-th entry once the list is full
    int thr_j = INT32_MAX;
    for (int t = 0; t < ntile; ++t) {
        if (t + 1 < ntile) fetch(t + 1);               // in flight during this tile's counts
        const unsigned *tp = tile + (t & 1) * kTile * WR;
        const int *bp = bs + (t & 1) * kTile;
        const int64_t c0 = pb + int64_t(t) * kTile;
        float key[16];
#pragma unroll
        for (int r = 0; r < kTile; ++r) {
            int c = 0;
#pragma unroll
            for (int w = 0; w < WR; ++w) c += __popc(q[w] & tp[r * WR + w]);
            const int u = qa + bp[r] - c;
            key[r] = u > 0 ? float(c) / float(u) : 0.f;
        }
        // ---- selection (offer_tile, topk_heap.h): a row past the part or the query's own index is no candidate
        offer_tile(key, row_ok, scr, ls, lj, lane, k, cnt, thr, thr_j, [&](int r, float) {
            const int64_t jj = c0 + r;
            if (jj >= pe) return -1;
            return a.excl_same && int(jj) == i ? -1 : int(jj);
        });
        if (t + 1 < ntile) stash(t + 1);               // the buffer tile t - 1 read; every wave is past that barrier
        __syncthreads();
    }
    heap_sort(ls, lj, lane, cnt);
    if (row_ok) {
        const bool direct = a.S == 1;
        float *os = direct ? a.value_out + i64 * a.ldo : a.part_s + (int64_t(split) * a.m + i64) * k;
        int32_t *oj = direct ? a.index_out + i64 * a.ldo : a.part_j + (int64_t(split) * a.m + i64) * k;
        merge_halves(ls, lj, lane, k, cnt, 0, [&](int t, float s, int j) { os[t] = s; oj[t] = j; });
    }
}

template <int WR>
int launch_sweep(int64_t blocks, size_t lds, hipStream_t st, const TaniArgs &a)
{
    return gae::launch_lds<&tanimoto_kernel<WR>>("tanimoto_kernel", blocks, kQueries, lds, st, a);
}

} // namespace

extern "C" int64_t gae_tanimoto_knn_workspace_bytes(int64_t m, int64_t n, int64_t n_words, int64_t k, int splits)
{
    Plan<int32_t> p;
    if (const int rc = plan("gae_tanimoto_knn_workspace_bytes", m, n, n_words, k, splits, nullptr, p)) return rc;
    return p.need;
}

extern "C" int gae_tanimoto_knn(const int32_t *Q, int64_t ldq, int64_t m, const int32_t *X, int64_t ldx, int64_t n,
                                int64_t n_words, int64_t k, int flags, int splits, int32_t *index_out, float *value_out,
                                int64_t ldo, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "gae_tanimoto_knn";
    Plan<int32_t> p;
    if (const int rc = plan(fn, m, n, n_words, k, splits, workspace, p)) return rc;
    if (const int rc = check_call(fn, "n_words", n_words, flags, ldq, ldx, ldo, m, n, k, Q, X, index_out, value_out,
                                  workspace, workspace_bytes, p.need))
        return rc;
    if (m == 0) return GAE_OK;

    const int S = splits_of(m, n, kQueries, splits);
    TaniArgs a;
    fill(a, ldq, ldx, ldo, m, n, k, S, flags, value_out, index_out, p.part);
    a.Q = Q; a.X = X; a.W = int(n_words);
    a.bcount = p.rows;
    hipStream_t st = gae::as_stream(stream);

    // every grid of the call, before the first launch
    const int64_t blocks = cdiv(m, kQueries) * S, merge_blocks = cdiv(m * S * k, 256);
    GAE_REQUIRE(blocks < (int64_t(1) << 31) && merge_blocks < (int64_t(1) << 31), GAE_E_SIZE,
                "%s: a grid of %lld / %lld blocks", fn, (long long)blocks, (long long)merge_blocks);
    if (n > 0) {
        hipLaunchKernelGGL(tanimoto_count_kernel, dim3(unsigned(cdiv(n, 256))), dim3(256), 0, st, X, ldx, int(n),
                           int(n_words), p.rows);
        GAE_CHECK_LAUNCH("tanimoto_count_kernel");
    }
    const size_t lds = size_t(sweep_lds(n_words, k));
    int rc = GAE_OK;
    switch (wr_of(n_words)) {
    case 1: rc = launch_sweep<1>(blocks, lds, st, a); break;
    case 2: rc = launch_sweep<2>(blocks, lds, st, a); break;
    case 4: rc = launch_sweep<4>(blocks, lds, st, a); break;
    case 8: rc = launch_sweep<8>(blocks, lds, st, a); break;
    case 16: rc = launch_sweep<16>(blocks, lds, st, a); break;
    case 32: rc = launch_sweep<32>(blocks, lds, st, a); break;
    default: rc = launch_sweep<64>(blocks, lds, st, a); break;
    }
    if (rc) return rc;
    if (S > 1) {
        const MergeArgs<int32_t> ma{a.part_s, a.part_j, m, a.k, S, value_out, index_out, ldo};
        hipLaunchKernelGGL(merge_kernel<int32_t>, dim3(unsigned(merge_blocks)), dim3(256), 0, st, ma);
        GAE_CHECK_LAUNCH("tanimoto_merge_kernel");
    }
    return GAE_OK;
}
