// What the entry points of the row searches K24 gae_knn (knn.hip) and K34 gae_tanimoto_knn (tanimoto.hip) share, once:
// the split rule and the workspace walk that goes with it, the argument checks in the order callers have seen them and
// the kernels' common arguments.  The kernels, their launches and their dispatch stay in their files.
#pragma once
#include "decoder_pairs.h"

namespace gae {
namespace search {

using pairs::kMaxSplits;
constexpr int kMaxK = 64, kTargetBlocks = 1024;        // kTargetBlocks: the auto split aims at four blocks per CU

struct SearchArgs {                        // KnnArgs and TaniArgs start with it; the operands are theirs
    int64_t ldq, ldx, ldo;
    int m, n, k, S, excl_same;
    float *value_out;
    int32_t *index_out;
    float *part_s;                         // [S][m][k] (S > 1)
    int32_t *part_j;
};

// column splits per block of `rows_per_block` queries: the caller's, or (0 = auto) enough for ~kTargetBlocks blocks with
// parts of >= 256 rows
static inline int splits_of(int64_t m, int64_t n, int64_t rows_per_block, int splits)
{
    if (splits > 0) return splits;
    if (m <= 0 || n <= 0) return 1;
    int64_t S = cdiv(kTargetBlocks, cdiv(m, rows_per_block));
    const int64_t by_span = cdiv(n, 256);
    S = S < by_span ? S : by_span;
    return int(S < 1 ? 1 : (S > kMaxSplits ? kMaxSplits : S));
}

// entries of the partial lists the workspace holds: a bound of S m that never shrinks as m, n or splits grow
// (auto: S <= kTargetBlocks / blocks + 1 and m <= most_rows_per_block blocks, S <= 16, S <= ceil(n / 256))
static inline int64_t part_rows(int64_t m, int64_t n, int splits, int64_t most_rows_per_block)
{
    if (splits > 0) return int64_t(splits) * m;
    int64_t b = int64_t(kMaxSplits) * m;
    const int64_t by_blocks = kTargetBlocks * most_rows_per_block + m, by_span = cdiv(n, 256) * m;
    b = b < by_blocks ? b : by_blocks;
    return b < by_span ? b : by_span;
}

// The workspace regions (NULL for the size query), behind what the size query checks: [n] words of the kernel's own
// (|x|^2 / 2, bit counts), then the partial lists (scores, then indices).  `width`: d or n_words, named `width_name`
template <class W> struct Plan { W *rows; float *part; int64_t need; };
template <class W>
static inline int carve(const char *fn, const char *width_name, int64_t width, int max_width, int64_t m, int64_t n,
                        int64_t k, int splits, int64_t most_rows_per_block, void *ws, Plan<W> &p)
{
    GAE_REQUIRE(width >= 1 && width <= max_width, GAE_E_RANGE, "%s: %s = %lld outside 1..%d", fn, width_name,
                (long long)width, max_width);
    GAE_REQUIRE(k >= 1 && k <= kMaxK, GAE_E_RANGE, "%s: k = %lld outside 1..64", fn, (long long)k);
    GAE_REQUIRE(m >= 0 && n >= 0, GAE_E_SIZE, "%s: negative m = %lld or n = %lld", fn, (long long)m, (long long)n);
    GAE_REQUIRE(m < (int64_t(1) << 31) && n < (int64_t(1) << 31), GAE_E_SIZE, "%s: m = %lld or n = %lld beyond int32 indices",
                fn, (long long)m, (long long)n);
    GAE_REQUIRE(splits >= 0 && splits <= kMaxSplits, GAE_E_RANGE, "%s: splits = %d outside 0..16", fn, splits);
    Carver c(ws);
    p.rows = c.take<W>(n);
    p.part = c.take<float>(2 * part_rows(m, n, splits, most_rows_per_block) * k);
    p.need = c.bytes() + 256;
    return GAE_OK;
}

// a real call, after carve: the leading dimensions, the arrays, and the workspace against the `need` of the size query
static inline int check_call(const char *fn, const char *width_name, int64_t width, int flags, int64_t ldq, int64_t ldx,
                             int64_t ldo, int64_t m, int64_t n, int64_t k, const void *Q, const void *X,
                             const void *index_out, const void *value_out, const void *workspace, int64_t workspace_bytes,
                             int64_t need)
{
    GAE_REQUIRE((flags & ~GAE_KNN_EXCLUDE_SAME_INDEX) == 0, GAE_E_RANGE, "%s: unknown flags 0x%x", fn, flags);
    GAE_REQUIRE(ldq >= width && ldx >= width && ldo >= k, GAE_E_SIZE,
                "%s: leading dimension too small (ldq %lld < %s, ldx %lld < %s or ldo %lld < k)", fn, (long long)ldq,
                width_name, (long long)ldx, width_name, (long long)ldo);
    GAE_REQUIRE(m == 0 || (index_out && value_out), GAE_E_NULL, "%s: index_out / value_out is NULL", fn);
    GAE_REQUIRE(m == 0 || Q, GAE_E_NULL, "%s: Q is NULL", fn);
    GAE_REQUIRE(m == 0 || n == 0 || X, GAE_E_NULL, "%s: X is NULL", fn);
    GAE_REQUIRE(workspace, GAE_E_NULL, "%s: workspace is NULL", fn);
    GAE_REQUIRE(workspace_bytes >= need, GAE_E_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn,
                (long long)workspace_bytes, (long long)need);
    return GAE_OK;
}

// the kernels' view of a checked call cut into S column splits; `part`: the partial lists, scores then indices
static inline void fill(SearchArgs &a, int64_t ldq, int64_t ldx, int64_t ldo, int64_t m, int64_t n, int64_t k, int S,
                        int flags, float *value_out, int32_t *index_out, float *part)
{
    a.ldq = ldq; a.ldx = ldx; a.ldo = ldo;
    a.m = int(m); a.n = int(n); a.k = int(k); a.S = S;
    a.excl_same = (flags & GAE_KNN_EXCLUDE_SAME_INDEX) ? 1 : 0;
    a.value_out = value_out; a.index_out = index_out; a.part_s = part;
    a.part_j = reinterpret_cast<int32_t *>(part + (S > 1 ? int64_t(S) * m * k : 0));
}

} // namespace search
} // namespace gae
