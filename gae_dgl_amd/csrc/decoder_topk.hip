// K16: top-k link prediction without the N x N matrix (GAE.predict_links, ops.decoder_topk).
//
// For every row i the k candidates j with the largest logit s_ij = z_i . z_j (gae_dgl/gae.py:69-72 without dropout and
// before the sigmoid).  Rows are sorted by (score descending, j ascending).  Who is a candidate, how the columns are
// split over waves and which bits s_ij has: decoder_pairs.h, shared with K18, K22, K23 and K24.
//
// Products.  The panel's rows stay in registers; the tiles of Z are loaded straight from global memory (L2-resident at
// every size measured), each feature behind its own bounds test.  Every lane's 16 scores belong to ONE row, so the
// threshold test needs no cross-lane traffic.
//
// Selection (topk_heap.h, shared with K24 and K34: offer_tile, merge_halves, merge_kernel).  Each lane keeps a running
// top-k of its (row, lane half) in LDS as a heap with the worst entry at the root.  Per tile the fast path is the max
// of the lane's 16 scores against the lane's k-th score (about 0.5 VALU op per pair); only lanes with a passing score
// store the tile to an LDS scratch row and walk the passing columns: window, self, a 64-bit hash of the CSR row (the
// row's indices are scanned only on a hash hit; any order, repeats allowed) and the heap insert. One heapsort at the
// end turns each heap into a list sorted best first. NaN and -inf never pass (the threshold starts at -FLT_MAX).
//
// Output.  The two lane halves of a row merge their lists in the wave.  With one column split the merged list is the
// row of the output; with S > 1 splits every (panel, split) wave writes a sorted partial list to the workspace and a
// second launch merges the S lists of each row by rank (binary search in the other lists): no atomics, and since the
// total order is strict the result is unique, so every schedule gives the same bits.
#include <float.h>
#include <string.h>

#include "decoder_pairs.h"
#include "topk_heap.h"

namespace {

using namespace gae::pairs;
using namespace gae::topk;

constexpr int kMaxK = 64;

struct TopkArgs : Common {
    int k;
    float *score_out;
    int64_t *index_out;
    int64_t ldo;
    float *part_s;                // [S][n][k] (S > 1)
    int32_t *part_j;
};

__device__ __forceinline__ unsigned hash6(int j) { return (unsigned(j) * 0x9E3779B1u) >> 26; }

template <int DH, bool ONE>
__global__ __launch_bounds__(64) void topk_kernel(const TopkArgs a)
{
    extern __shared__ float lds[];
    const int lane = threadIdx.x, col = lane & 31, h = lane >> 5;
    const int k = a.k;
    float *ls = lds;                                       // [k][64] scores of each lane's list
    int *lj = reinterpret_cast<int *>(lds + k * 64);       // [k][64] indices
    float *scr = lds + 2 * k * 64;                         // [16][64] scores of a tile that has a passing lane
    const int panel = blockIdx.x / a.S, split = blockIdx.x % a.S;
    const int i = panel * kRows + col;
    const bool row_ok = i < a.n;

    // ---- the row: member window, CSR row, hash of its indices
    int w0 = 0, w1 = 0;
    if (row_ok) member_window(a, i, w0, w1);
    int e0 = 0, e1 = 0;
    unsigned long long hmask = 0;
    if (row_ok && a.indptr) {
        e0 = a.indptr[i]; e1 = a.indptr[i + 1];
        for (int e = e0; e < e1; ++e) hmask |= 1ull << hash6(a.indices[e]);
    }
    // ---- the wave's column part and this lane's candidates in it
    int pb, pe, lo, hi;
    wave_part(w0, w1, a.S, split, pb, pe, lo, hi);

    // ---- the panel rows (B operand)
    float zr[DH];
    auto load_row = [&](int q) {
#pragma unroll
        for (int s = 0; s < DH; ++s) {
            const int f = feat0<DH>(q, h) + s;
            zr[s] = (row_ok && f < a.d) ? a.Z[int64_t(i) * a.ldz + f] : 0.f;
        }
    };
    if constexpr (ONE) load_row(0);

    int cnt = 0;
    float thr = -FLT_MAX;                          // score of the k-th entry once the list is full
    int thr_j = INT32_MAX;
    for (int64_t c0_ = pb; c0_ < pe; c0_ += kTile) {
        const int c0 = int(c0_);
        v16f acc = zero_acc();
        const int64_t jc = int64_t(c0) + col;      // this lane's A-operand column (int64: n may reach 2^31 - 1)
        const bool col_ok = jc < pe;
        for (int q = 0; q < (ONE ? 1 : a.nch); ++q) {
            if constexpr (!ONE) load_row(q);
            float za[DH];
#pragma unroll
            for (int s = 0; s < DH; ++s) {
                const int f = feat0<DH>(q, h) + s;
                za[s] = (col_ok && f < a.d) ? a.Z[jc * a.ldz + f] : 0.f;
            }
            acc = mma<DH>(acc, za, zr);
        }
        // ---- selection (offer_tile, topk_heap.h): window and self before the threshold, the CSR row -- scanned on a
        // hash hit only -- after it
        offer_tile(
            acc, lo < hi, scr, ls, lj, lane, k, cnt, thr, thr_j,
            [&](int r, float) {
                const int64_t jj = tile_col(int64_t(c0), r, h);
                if (jj < lo || jj >= hi) return -1;
                return a.excl_self && int(jj) == i ? -1 : int(jj);
            },
            [&](int j) { return !(((hmask >> hash6(j)) & 1ull) && row_holds(a.indices, e0, e1, j)); });
    }
    // ---- the heap into a list sorted best first: the worst entry goes to the end, k log k steps once
    heap_sort(ls, lj, lane, cnt);
    // ---- merge the two lane halves of each row; lane h = 0 writes the row
    __syncthreads();
    const int pcnt = __shfl_down(cnt, 32, 64);
    if (h == 0 && row_ok) {
        const bool direct = a.S == 1;
        float *os = direct ? a.score_out + int64_t(i) * a.ldo : a.part_s + (int64_t(split) * a.n + i) * k;
        int64_t *oj64 = a.index_out + int64_t(i) * a.ldo;
        int32_t *oj32 = a.part_j + (int64_t(split) * a.n + i) * k;
        merge_halves(ls, lj, lane, k, cnt, pcnt, [&](int t, float s, int j) {
            os[t] = s;
            if (direct) oj64[t] = j; else oj32[t] = j;
        });
    }
}

int64_t need_bytes(int64_t n, int64_t k, int S) { return S > 1 ? int64_t(S) * n * k * 8 + 256 : 256; }

} // namespace

namespace gae {
Knob g_topk_splits{0};       // "topk_splits": column splits per panel, 0 = auto (tests force 1 or more)
} // namespace gae

extern "C" int gae_decoder_topk(const float *Z, int64_t ldz, int64_t n, int64_t d, int64_t k, const int64_t *node_ptr,
                                int64_t n_graphs, int64_t max_graph_nodes, const int32_t *indptr,
                                const int32_t *indices, int flags, float *score_out, int64_t *index_out, int64_t ldo,
                                void *workspace, int64_t *workspace_bytes, void *stream)
{
    const char *fn = "gae_decoder_topk";
    const Request r{Z, ldz, n, d, node_ptr, n_graphs, max_graph_nodes, indptr, indices, flags, workspace_bytes};
    GAE_REQUIRE(k >= 1 && k <= kMaxK, GAE_E_RANGE, "%s: k = %lld outside 1..64", fn, (long long)k);
    // both leading dimensions in one message, ahead of the common ldz check: the text callers have seen since K16
    GAE_REQUIRE(ldz >= d && ldo >= k, GAE_E_SIZE, "%s: leading dimension too small (ldz %lld < d or ldo %lld < k)", fn,
                (long long)ldz, (long long)ldo);
    if (const int rc = check_sizes(fn, r)) return rc;
    const int64_t panels = (n + kRows - 1) / kRows;
    const int S = splits(panels, n, node_ptr, max_graph_nodes, gae::g_topk_splits);
    const int64_t need = need_bytes(n, k, S);
    if (!workspace) {                               // size query: no device work
        *workspace_bytes = need;
        return GAE_OK;
    }
    GAE_REQUIRE(n == 0 || (score_out && index_out), GAE_E_NULL, "%s: score_out / index_out is NULL", fn);
    if (const int rc = check_arrays(fn, r, need)) return rc;
    if (n == 0) return GAE_OK;
    TopkArgs a;
    fill(a, r, S);
    a.k = int(k); a.score_out = score_out; a.index_out = index_out; a.ldo = ldo;
    a.part_s = reinterpret_cast<float *>(static_cast<char *>(workspace) + 256);
    a.part_j = reinterpret_cast<int32_t *>(a.part_s + (S > 1 ? int64_t(S) * n * k : 0));
    const size_t lds = size_t(lists_bytes(int(k)));
    hipStream_t st = gae::as_stream(stream);
    dispatch(d, [&](auto dh, auto one) {
        hipLaunchKernelGGL((topk_kernel<dh, one>), dim3(unsigned(panels * S)), dim3(64), lds, st, a);
    });
    GAE_CHECK_LAUNCH("topk_kernel");
    if (S > 1) {
        const int64_t threads = n * S * k;
        const MergeArgs<int64_t> ma{a.part_s, a.part_j, n, a.k, S, score_out, index_out, ldo};
        hipLaunchKernelGGL(merge_kernel<int64_t>, dim3(unsigned((threads + 255) / 256)), dim3(256), 0, st, ma);
        GAE_CHECK_LAUNCH("topk_merge_kernel");
    }
    return GAE_OK;
}
