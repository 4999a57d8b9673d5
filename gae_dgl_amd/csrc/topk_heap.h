// The selection helpers of the k-best kernels: K16 gae_decoder_topk (decoder_topk.hip) and K24 gae_knn (knn.hip).
// One total order (larger value first, then the lower index), a per-lane heap in LDS with the WORST entry at the root,
// and the rank of an entry in a sorted partial list, by which the lists of the column splits are merged.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace gae {
namespace topk {

// (s, j) is better than (t, q): the total order of the output (score descending, then j ascending)
__device__ __forceinline__ bool better(float s, int j, float t, int q) { return s > t || (s == t && j < q); }

// Each lane's running top-k is a binary heap in LDS (entry p of lane l at [p * 64 + l]) with the WORST entry at the
// root: the threshold is the root, and an insert costs log2 k dependent LDS round trips instead of the k / 2 of a
// shift into a sorted list.
__device__ __forceinline__ void heap_push(float *ls, int *lj, int lane, int cnt, float s, int j)
{
    int p = cnt;
    while (p > 0) {                                // sift up past every parent that is better than the new entry
        const int q = (p - 1) >> 1;
        const float t = ls[q * 64 + lane];
        const int tj = lj[q * 64 + lane];
        if (!better(t, tj, s, j)) break;
        ls[p * 64 + lane] = t;
        lj[p * 64 + lane] = tj;
        p = q;
    }
    ls[p * 64 + lane] = s;
    lj[p * 64 + lane] = j;
}

// replace the root of a heap of `size` entries by (s, j) and sift it down
__device__ __forceinline__ void heap_replace_root(float *ls, int *lj, int lane, int size, float s, int j)
{
    int p = 0;
    while (true) {
        int c = 2 * p + 1;
        if (c >= size) break;
        float cs = ls[c * 64 + lane];
        int cj = lj[c * 64 + lane];
        if (c + 1 < size) {
            const float ds = ls[(c + 1) * 64 + lane];
            const int dj = lj[(c + 1) * 64 + lane];
            if (better(cs, cj, ds, dj)) { cs = ds; cj = dj; c = c + 1; }     // the worse child
        }
        if (!better(s, j, cs, cj)) break;          // (s, j) is no better than its worse child: it stays here
        ls[p * 64 + lane] = cs;
        lj[p * 64 + lane] = cj;
        p = c;
    }
    ls[p * 64 + lane] = s;
    lj[p * 64 + lane] = j;
}

// the heap of `cnt` entries into a list sorted best first: the worst entry goes to the end, k log k steps once
__device__ __forceinline__ void heap_sort(float *ls, int *lj, int lane, int cnt)
{
    for (int e = cnt - 1; e > 0; --e) {
        const float ts = ls[e * 64 + lane];
        const int tj = lj[e * 64 + lane];
        const float rs = ls[lane];
        const int rj = lj[lane];
        ls[e * 64 + lane] = rs;
        lj[e * 64 + lane] = rj;
        heap_replace_root(ls, lj, lane, e, ts, tj);
    }
}

// entries of a sorted partial list (length k, padding j = -1 at the end) better than (s, j)
__device__ __forceinline__ int rank_in(const float *ps, const int32_t *pj, int k, float s, int j)
{
    int l = 0, h = k;                              // first position that is not better
    while (l < h) {
        const int m = (l + h) >> 1;
        const bool b = pj[m] >= 0 && better(ps[m], pj[m], s, j);
        if (b) l = m + 1; else h = m;
    }
    return l;
}

__device__ __forceinline__ int valid_in(const int32_t *pj, int k)
{
    int l = 0, h = k;
    while (l < h) { const int m = (l + h) >> 1; if (pj[m] >= 0) l = m + 1; else h = m; }
    return l;
}

} // namespace topk
} // namespace gae
