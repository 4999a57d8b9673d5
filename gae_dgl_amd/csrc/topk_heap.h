// The k-best tail of K16 gae_decoder_topk, K24 gae_knn and K34 gae_tanimoto_knn (decoder_topk.hip, knn.hip,
// tanimoto.hip), from a lane's 16 keys of a tile to the output row: one total order (larger value first, then the lower
// index); a per-lane heap in LDS with the WORST entry at the root; offer_tile, the walk that feeds it the keys of a
// tile that pass the running threshold, with the kernel's own candidate tests as hooks; merge_halves, the merge of the
// two lane halves of a row; and merge_kernel, the second launch that merges the sorted partial lists of the column
// splits by rank.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace gae {
namespace topk {

// (s, j) is better than (t, q): the total order of the output (score descending, then j ascending)
__device__ __forceinline__ bool better(float s, int j, float t, int q) { return s > t || (s == t && j < q); }
// the same order over an integer key (K36: an int64 count or sum, or the bits of a non-negative fp64 quotient)
__device__ __forceinline__ bool better(int64_t s, int j, int64_t t, int q) { return s > t || (s == t && j < q); }

// LDS of one wave: ls [k][64] and lj [k][64], the lists of its 64 lanes, and scr [16][64], the scratch rows of offer_tile
constexpr int lists_bytes(int k) { return (2 * k + 16) * 256; }

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

// what offer_tile's second hook is when a kernel has none
struct EveryIndex {
    __device__ __forceinline__ bool operator()(int) const { return true; }
};

// The 16 keys of a lane's tile against its running top k: the heap (ls, lj) of cnt entries, (thr, thr_j) its k-th
// entry once it is full (before that thr = -FLT_MAX: NaN and -inf never pass).  The fast path is one max per key and
// one compare per tile; only a `live` lane with a passing key spills the tile to its column of the scratch rows scr
// ([16][64]) and walks the passing keys in register order.  index_of(r, key) gives the candidate's index, or a negative
// number when register r holds none; it runs BEFORE the test against the threshold, keep(j) (a dearer test, such as a
// CSR lookup) only after it
template <class Keys, class IndexOf, class Keep = EveryIndex>
__device__ __forceinline__ void offer_tile(const Keys &key, bool live, float *scr, float *ls, int *lj, int lane, int k,
                                           int &cnt, float &thr, int &thr_j, IndexOf &&index_of, Keep &&keep = Keep())
{
    float m = key[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) m = fmaxf(m, key[r]);
    if (!(m >= thr && live)) return;
    unsigned pass = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        scr[r * 64 + lane] = key[r];
        pass |= (key[r] >= thr ? 1u : 0u) << r;
    }
    while (pass) {
        const int r = __builtin_ctz(pass);
        pass &= pass - 1;
        const float s = scr[r * 64 + lane];
        const int j = index_of(r, s);
        if (j < 0) continue;
        if (cnt == k && !better(s, j, thr, thr_j)) continue;
        if (!keep(j)) continue;
        if (cnt < k) {
            heap_push(ls, lj, lane, cnt, s, j);
            ++cnt;
        } else {
            heap_replace_root(ls, lj, lane, k, s, j);
        }
        if (cnt == k) {
            thr = ls[lane];
            thr_j = lj[lane];
        }
    }
}

// the two sorted lists of a row -- cnt entries of `lane` (lane half 0, the caller) and pcnt of lane + 32 -- merged into
// k entries best first, padding (-inf, -1) at the end: store(t, s, j) for t = 0 .. k - 1
template <class Store>
__device__ __forceinline__ void merge_halves(const float *ls, const int *lj, int lane, int k, int cnt, int pcnt,
                                             Store &&store)
{
    int p0 = 0, p1 = 0;
    for (int t = 0; t < k; ++t) {
        float s = -INFINITY;
        int j = -1;
        const bool h0 = p0 < cnt, h1 = p1 < pcnt;
        if (h0 || h1) {
            const float s0 = h0 ? ls[p0 * 64 + lane] : 0.f, s1 = h1 ? ls[p1 * 64 + lane + 32] : 0.f;
            const int j0 = h0 ? lj[p0 * 64 + lane] : 0, j1 = h1 ? lj[p1 * 64 + lane + 32] : 0;
            if (h0 && (!h1 || better(s0, j0, s1, j1))) { s = s0; j = j0; ++p0; }
            else { s = s1; j = j1; ++p1; }
        }
        store(t, s, j);
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

// ---- the second launch of a call with S > 1 column splits
template <class Index>
struct MergeArgs {
    const float *part_s;          // [S][rows][k]: the sorted partial lists
    const int32_t *part_j;
    int64_t rows;
    int k, S;
    float *score_out;             // [rows][ldo]
    Index *index_out;
    int64_t ldo;
};

// one thread per (row, split, position): the entry's rank among the S lists of its row is its output slot.  The order
// is total and strict, so the result is unique: no atomics, and every schedule and every S give the same bits
template <class Index>
__global__ __launch_bounds__(256) void merge_kernel(const MergeArgs<Index> a)
{
    const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
    const int k = a.k, S = a.S;
    if (t >= a.rows * S * k) return;
    const int q = int(t % k);
    const int s = int((t / k) % S);
    const int64_t i = t / (int64_t(k) * S);
    const int64_t stride = a.rows * k;
    const float *ps = a.part_s + i * k;
    const int32_t *pj = a.part_j + i * k;
    float *os = a.score_out + i * a.ldo;
    Index *oj = a.index_out + i * a.ldo;
    const int j = pj[s * stride + q];
    if (j >= 0) {
        const float v = ps[s * stride + q];
        int rank = q;
        for (int u = 0; u < S; ++u)
            if (u != s) rank += rank_in(ps + u * stride, pj + u * stride, k, v, j);
        if (rank < k) { os[rank] = v; oj[rank] = j; }
    }
    if (s == 0) {
        int total = 0;
        for (int u = 0; u < S; ++u) total += valid_in(pj + u * stride, k);
        if (q >= total) { os[q] = -INFINITY; oj[q] = -1; }
    }
}

} // namespace topk
} // namespace gae
