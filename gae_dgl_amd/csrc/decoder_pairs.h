// The pair scores of the kernels on the 32 x 32 product tile: K16 gae_decoder_topk (decoder_topk.hip), K18
// gae_decoder_rank (decoder_rank.hip), K22 gae_decoder_threshold_* (decoder_threshold.hip), K23 gae_kmeans_*
// (kmeans.hip) and K24 gae_knn (knn.hip).  K18 ranks a pair against the number K16 lists for it, K22 lists that number,
// and K24 with Q = X has its bits, so they must give a pair the SAME bits and the same candidates.  What decides either
// lives here, once: the same code, not copies that agree.  Each kernel keeps its own selection, counting or compaction
// and its later launches; K16, K23 and K24 also keep their own operand loads (straight from global memory, an LDS image
// of C, LDS-staged tiles of X).
//
// Candidates (include/gae_hip.h).  Column c is a candidate of row i when it lies in i's column window -- all n without
// node_ptr, else i's own member [node_ptr[g], node_ptr[g + 1]) clipped to [0, n) (member_window; a row outside every
// member has none) --, c != i under GAE_TOPK_EXCLUDE_SELF, c is not in CSR row i under GAE_TOPK_EXCLUDE_EDGES (any
// order, repeats allowed: row_holds), and s_ic is neither NaN nor -inf.  K18 and K22 decide window, self and validity
// per tile through LaneTile: the fast path of a tile that needs no per-column test, else one predicate per column.
//
// Work split.  One wave per panel of kRows rows and column split.  The wave's columns are the union of its rows'
// windows, cut into S parts of whole tiles (wave_part); a lane's own candidates are its row's window inside that part.
//
// Operands.  The panel's rows are the B operand of v_mfma_f32_32x32x2_f32, tiles of kTile rows of Z the A operand.
// A lane (row or column l & 31, half h = l >> 5) feeds the DH features feat0<DH>(ch, h) + s, s = 0 .. DH - 1, of each
// 2 DH-wide chunk ch, one MFMA per s (mma<DH>), chunks ascending; d picks DH and the chunk count (dispatch, dh_of,
// chunks_of).  Accumulator register r of lane l then holds row l & 31 against column tile_col(c0, r, l >> 5) of the tile
// (tile_owner is the inverse): all 16 scores of a lane belong to ONE row.  The f32 MFMA is bitwise a k-ordered fmaf
// chain from 0.f, and this feature order is fixed, so s_ic depends only on the bits of z_i and z_c -- not on where c
// falls in a tile, which split sweeps it or which of the kernels asks.  Equal rows give bit-equal scores, K16's
// tie rule is exact, and K18's "s_ic == t" compares bits of one and the same chain.
//
// The sweep of K18 and K22 (load_feats, sweep_tiles): operand loads without branches -- row and feature clamped, tail
// features zeroed -- and, with one chunk, the next tile's loads issued before the current tile is used.
#pragma once
#include <type_traits>

#include "common.h"

namespace gae {
namespace pairs {

constexpr int kRows = 32;         // panel rows (K16) or queries (K18) per wave
constexpr int kTile = 32;         // columns per tile
constexpr int kMaxSplits = 16;

typedef float v16f __attribute__((ext_vector_type(16)));

struct Common {                   // TopkArgs and RankArgs start with it
    const float *Z;
    int64_t ldz;
    int n, d, nch, S;
    const int64_t *node_ptr;      // NULL = scope batch
    int64_t G;
    const int32_t *indptr, *indices;      // NULL without GAE_TOPK_EXCLUDE_EDGES
    int excl_self;
};

// the member window [w0, w1) of row i (empty when i lies outside every member)
__device__ __forceinline__ void member_window(const Common &a, int i, int &w0, int &w1)
{
    if (!a.node_ptr) { w0 = 0; w1 = a.n; return; }
    w0 = 0; w1 = 0;
    if (a.G <= 0 || a.node_ptr[0] > i) return;
    int64_t l = 0, h = a.G;                       // last member g < G with node_ptr[g] <= i
    while (h - l > 1) { const int64_t m = (l + h) >> 1; if (a.node_ptr[m] <= i) l = m; else h = m; }
    int64_t p0 = a.node_ptr[l], p1 = a.node_ptr[l + 1];
    p0 = p0 < 0 ? 0 : p0;                         // clipped to [0, n): a bad node_ptr never reads outside Z
    p1 = p1 > a.n ? a.n : p1;
    if (i >= p0 && i < p1) { w0 = int(p0); w1 = int(p1); }
}

// the wave's column part [pb, pe) -- the union of its 32 rows' windows [w0, w1), cut into S tile-aligned parts, part
// `split` -- and the lane's candidates [lo, hi): its row's window inside that part.  pb, pe: the same in every lane
__device__ __forceinline__ void wave_part(int w0, int w1, int S, int split, int &pb, int &pe, int &lo, int &hi)
{
    int cb = w0 < w1 ? w0 : INT32_MAX, ce = w0 < w1 ? w1 : INT32_MIN;
    for (int off = 32; off > 0; off >>= 1) {
        const int ob = __shfl_xor(cb, off, 64), oe = __shfl_xor(ce, off, 64);
        cb = ob < cb ? ob : cb;
        ce = oe > ce ? oe : ce;
    }
    pb = 0; pe = 0;
    if (cb < ce) {
        const int64_t span = int64_t(ce) - cb;
        const int64_t L = ((span + S - 1) / S + kTile - 1) / kTile * kTile;
        const int64_t b = cb + L * split, e = b + L;
        pb = int(b < ce ? b : ce);
        pe = int(e < ce ? e : ce);
    }
    lo = w0 > pb ? w0 : pb; hi = w1 < pe ? w1 : pe;
}

// the first of the DH features lane half h feeds from chunk ch
template <int DH>
__device__ __forceinline__ int feat0(int ch, int h) { return ch * 2 * DH + h * DH; }

// the column of accumulator register r in lane half h, for the tile whose first column is c0 (0: the column inside the
// tile).  Summed in c0's type: K16 passes an int64 column (n may reach 2^31 - 1) ...
template <class T>
__device__ __forceinline__ T tile_col(T c0, int r, int h) { return c0 + (r & 3) + 8 * (r >> 2) + 4 * h; }

// ... and its inverse: the lane and register that hold `row` against column c of the tile
__device__ __forceinline__ void tile_owner(int row, int c, int &lane, int &reg)
{
    lane = row + 32 * ((c >> 2) & 1);
    reg = (c & 3) + 4 * (c >> 3);
}

__device__ __forceinline__ v16f zero_acc()
{
    v16f acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    return acc;
}

// one chunk: acc += (tile rows za) x (panel rows zb) over the lane halves' 2 DH features
template <int DH>
__device__ __forceinline__ v16f mma(v16f acc, const float (&za)[DH], const float (&zb)[DH])
{
#pragma unroll
    for (int s = 0; s < DH; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(za[s], zb[s], acc, 0, 0, 0);
    return acc;
}

// ---- operand loads and the sweep of K18 and K22
// the DH features feat0<DH>(ch, h) + s of row `row` of Z (leading dimension ldz).  The caller clamps the row into [0, n)
// (the host launches nothing when n = 0) and the feature index is clamped here, so no load carries a branch.  A feature
// past d is zeroed: it would enter every product.  A clamped ROW is not: row c of the A operand reaches only the scores
// of column c, row r of the B operand only those of panel row r, and neither is used.  full: no_tail<DH>(a)
template <int DH>
__device__ __forceinline__ void load_feats(float (&z)[DH], const float *Z, int64_t ldz, int64_t row, int ch, int h, int d,
                                           bool full)
{
    const float *p = Z + row * ldz;
    const int f0 = feat0<DH>(ch, h);
    if (full) {
#pragma unroll
        for (int s = 0; s < DH; ++s) z[s] = p[f0 + s];
    } else {
#pragma unroll
        for (int s = 0; s < DH; ++s) {
            const int f = f0 + s;
            const float v = p[f < d ? f : d - 1];
            z[s] = f < d ? v : 0.f;
        }
    }
}

// no feature tail: the common d = 16, 32, 64, 128, 256
template <int DH>
__device__ __forceinline__ bool no_tail(const Common &a) { return a.d == a.nch * 2 * DH; }

// one tile: the rows of Z picked by `row` (in [0, n)) against panel row i.  The panel rows (B operand) stay in zr when
// one chunk holds all of d (ONE: the caller has loaded them), else they are loaded again per chunk
template <int DH, bool ONE>
__device__ __forceinline__ v16f tile_product(const Common &a, float (&zr)[DH], int i, int64_t row, int h, bool full)
{
    v16f acc = zero_acc();
    for (int ch = 0; ch < (ONE ? 1 : a.nch); ++ch) {
        if constexpr (!ONE) load_feats(zr, a.Z, a.ldz, i, ch, h, a.d, full);
        float za[DH];
        load_feats(za, a.Z, a.ldz, row, ch, h, a.d, full);
        acc = mma<DH>(acc, za, zr);
    }
    return acc;
}

// the tiles of the wave's part [pb, pe) (scalars: readfirstlane'd by the caller, so the loop control is scalar) against
// panel row i, on_tile(acc, c0) for each.  A column past the part is clamped into it
template <int DH, bool ONE, class OnTile>
__device__ __forceinline__ void sweep_tiles(const Common &a, float (&zr)[DH], int i, int col, int h, bool full, int pb,
                                            int pe, OnTile &&on_tile)
{
    const int64_t last = int64_t(pe) - 1;
    if constexpr (ONE) {
        // the next tile's A operand is in flight while this tile is multiplied and handed on
        float za[DH];
        if (pb < pe) load_feats(za, a.Z, a.ldz, int64_t(pb) + col < last ? int64_t(pb) + col : last, 0, h, a.d, full);
        for (int64_t c0 = pb; c0 < pe; c0 += kTile) {
            const v16f acc = mma<DH>(zero_acc(), za, zr);
            const int64_t jn = c0 + kTile + col;
            if (c0 + kTile < pe) load_feats(za, a.Z, a.ldz, jn < last ? jn : last, 0, h, a.d, full);
            on_tile(acc, int(c0));
        }
    } else {
        for (int64_t c0 = pb; c0 < pe; c0 += kTile) {
            const int64_t jc = c0 + col;           // this lane's A-operand column
            const v16f acc = tile_product<DH, false>(a, zr, i, jc < pe ? jc : last, h, full);
            on_tile(acc, int(c0));
        }
    }
}

// ---- the clean-tile rule of K18 and K22: which of a lane's 16 columns of the tile at c0 are candidates by window,
// excluded columns and validity (known edges are the kernel's own business), and may the tile skip the per-column test.
// Everything is relative to c0, so no column index leaves int32 (n may reach 2^31 - 1).
// the position in the tile at c0 of column x (-1: none); a result outside [0, kTile) is not in the tile
__device__ __forceinline__ int tile_rel(int x, int c0) { return x >= c0 ? x - c0 : -1; }

struct LaneTile {
    int lo_r, hi_r;                // the lane's candidates [lo, hi) inside the tile
    __device__ __forceinline__ LaneTile(int lo, int hi, int c0)
        : lo_r(lo > c0 ? lo - c0 : 0), hi_r(hi - c0 < kTile ? hi - c0 : kTile) {}
    // nothing of this lane's window in the tile
    __device__ __forceinline__ bool empty() const { return lo_r >= hi_r; }
    // the fast path: the tile lies inside the window, holds none of the excluded columns x_r (tile_rel), and its 16
    // scores are valid -- a NaN or a -inf among them makes the sum NaN or -inf
    template <class... X>
    __device__ __forceinline__ bool all_candidates(const v16f &acc, X... x_r) const
    {
        float sum = acc[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) sum += acc[r];
        const bool clean = lo_r == 0 && hi_r == kTile && (... && (unsigned(x_r) >= unsigned(kTile)));
        return clean && sum > -INFINITY;
    }
    // the masked path: is column c of the tile, with score s, a candidate?
    template <class... X>
    __device__ __forceinline__ bool candidate(int c, float s, X... x_r) const
    {
        return c >= lo_r && c < hi_r && (... && (c != x_r)) && s > -INFINITY;
    }
};

// does indices[b, e) hold v?  Four independent loads per round trip, clamped inside the stretch
__device__ __forceinline__ bool row_holds(const int32_t *indices, int b, int e, int v)
{
    bool hit = false;
    for (int x = b; x < e && !hit; x += 4) {
        const int32_t v0 = indices[x];
        const int32_t v1 = indices[x + 1 < e ? x + 1 : e - 1];
        const int32_t v2 = indices[x + 2 < e ? x + 2 : e - 1];
        const int32_t v3 = indices[x + 3 < e ? x + 3 : e - 1];
        hit = v0 == v || v1 == v || v2 == v || v3 == v;
    }
    return hit;
}

// ---- host side: the ladder from d to the kernel form -- one chunk of 2 DH >= d features whose panel rows stay in
// registers (ONE), or chunks of 64.  f(DH, ONE) gets both as compile-time constants (std::integral_constant,
// std::bool_constant), so a launch sits in a generic lambda: kernel<dh, one>
template <class F>
static inline auto dispatch(int64_t d, F &&f)
{
    if (d <= 16) return f(std::integral_constant<int, 8>{}, std::true_type{});
    if (d <= 32) return f(std::integral_constant<int, 16>{}, std::true_type{});
    if (d <= 64) return f(std::integral_constant<int, 32>{}, std::true_type{});
    return f(std::integral_constant<int, 32>{}, std::false_type{});
}
static inline int dh_of(int64_t d) { return dispatch(d, [](auto dh, auto) { return int(dh); }); }
static inline int chunks_of(int64_t d) { return int(cdiv(d, 2 * dh_of(d))); }

// ---- the column split and the entry points' common checks (static: the library exports nothing new) ------------------
// column splits per panel: the knob's value, or (0 = auto) enough to put ~4096 waves on the chip with parts of >= 256
// columns of the widest window
static inline int splits(int64_t panels, int64_t n, const int64_t *node_ptr, int64_t max_graph_nodes, int knob)
{
    if (n <= 0 || panels <= 0) return 1;
    int64_t S = knob;
    if (S <= 0) {
        const int64_t span = node_ptr ? (max_graph_nodes < n ? max_graph_nodes : n) : n;
        S = (4096 + panels - 1) / panels;                  // ~4096 waves: several per SIMD
        const int64_t by_span = (span + 255) / 256;        // parts of >= 256 columns
        S = S < by_span ? S : by_span;
    }
    return int(S < 1 ? 1 : (S > kMaxSplits ? kMaxSplits : S));
}

// what the two entry points ask of their common arguments; `fn` names the caller
struct Request {
    const float *Z;
    int64_t ldz, n, d;
    const int64_t *node_ptr;
    int64_t n_graphs, max_graph_nodes;
    const int32_t *indptr, *indices;
    int flags;
    const int64_t *workspace_bytes;
};

// before the size query: nothing is dereferenced
static inline int check_sizes(const char *fn, const Request &r)
{
    GAE_REQUIRE(r.d >= 1 && r.d <= 256, GAE_E_RANGE, "%s: d = %lld outside 1..256", fn, (long long)r.d);
    GAE_REQUIRE(r.n >= 0, GAE_E_SIZE, "%s: negative n = %lld", fn, (long long)r.n);
    GAE_REQUIRE(r.n < (int64_t(1) << 31), GAE_E_SIZE, "%s: n = %lld beyond the int32 CSR", fn, (long long)r.n);
    GAE_REQUIRE(r.ldz >= r.d, GAE_E_SIZE, "%s: leading dimension too small (ldz %lld < d)", fn, (long long)r.ldz);
    GAE_REQUIRE((r.flags & ~(GAE_TOPK_EXCLUDE_SELF | GAE_TOPK_EXCLUDE_EDGES)) == 0, GAE_E_RANGE,
                "%s: unknown flags 0x%x", fn, r.flags);
    GAE_REQUIRE(!r.node_ptr || (r.n_graphs >= 0 && r.max_graph_nodes >= 0), GAE_E_SIZE,
                "%s: negative n_graphs / max_graph_nodes", fn);
    GAE_REQUIRE(r.workspace_bytes, GAE_E_NULL, "%s: workspace_bytes is NULL", fn);
    return GAE_OK;
}

// a real call: the arrays, and the workspace against the `need` of the size query
static inline int check_arrays(const char *fn, const Request &r, int64_t need)
{
    GAE_REQUIRE(r.n == 0 || r.Z, GAE_E_NULL, "%s: Z is NULL", fn);
    GAE_REQUIRE(!(r.flags & GAE_TOPK_EXCLUDE_EDGES) || (r.indptr && r.indices), GAE_E_NULL,
                "%s: GAE_TOPK_EXCLUDE_EDGES without a CSR", fn);
    GAE_REQUIRE(*r.workspace_bytes >= need, GAE_E_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn,
                (long long)*r.workspace_bytes, (long long)need);
    return GAE_OK;
}

// the kernels' view of a checked request cut into S column splits; the CSR only when its rows are to be left out
static inline void fill(Common &a, const Request &r, int S)
{
    a.Z = r.Z; a.ldz = r.ldz; a.n = int(r.n); a.d = int(r.d); a.S = S;
    a.nch = chunks_of(r.d);
    a.node_ptr = r.node_ptr; a.G = r.n_graphs;
    const bool edges = (r.flags & GAE_TOPK_EXCLUDE_EDGES) != 0;
    a.indptr = edges ? r.indptr : nullptr; a.indices = edges ? r.indices : nullptr;
    a.excl_self = (r.flags & GAE_TOPK_EXCLUDE_SELF) ? 1 : 0;
}

} // namespace pairs
} // namespace gae
